"""Shared cases for the workgroup decode kernel with DM_UNPOPULATED /
DM_STRUCTURED (``test_wg_decode_host.py`` on the CPU build's host driver,
``test_gpu_wg_flags.py`` on gfx950).

A plain helper module, not a conftest.  Every case is (schema name, wire);
the reference is the classic kernel ``k_pb2json`` on the same wire with the
same mode: ``(status, bytes)`` must be equal.  ``GROUPS`` maps a group name to
a function of ``uc.Envs`` returning ``{case id: (schema name, wire)}``.
"""

from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import any_corpus as ac
import protojson_corpus as pc
import unpopulated_corpus as uc
from protojson_corpus import ld, tag

FLAG_SETS = (0, uc.DM_UNPOPULATED, uc.DM_UNPOPULATED | uc.DM_STRUCTURED)
BATCH = 96          # routed slots per batch: ~200 KB of scratch each

SPECIALS = '"\\\n\x01é😀'          # 10 bytes of UTF-8
SLICE = 4096                        # pb2json_wg.h wgd_slice


def tool_for(envs: uc.Envs, name: str) -> str:
    """Any tool of the engine that holds ``name``: primes the id slots."""
    if name in ("t.Sink", "bench.Wide64", "bench.Inner"):
        return envs.sink.sink_tool
    if name == "t.Holder":
        return envs.holder.tool
    return sorted(envs.infos)[0]


# ---- group 1: the corpora ------------------------------------------------------

def corpus(envs: uc.Envs) -> Dict[str, tuple]:
    out = dict(uc.corpus_wires(envs))
    for cid, (name, wire, _) in uc.targeted_cases(uc.sink_descriptor()).items():
        out[f"targeted:{cid}"] = (name, wire)
    return out


# ---- group 2: sparse bench.Wide64 ----------------------------------------------

def _wide(envs: uc.Envs, **kw):
    return envs.sink.wide_cls(**kw)


def _set_number(msg, number: int) -> None:
    fd = msg.DESCRIPTOR.fields_by_number[number]
    if fd.type in (fd.TYPE_STRING,):
        setattr(msg, fd.name, "sixty")
    elif fd.type == fd.TYPE_BYTES:
        setattr(msg, fd.name, b"sixty")
    elif fd.type == fd.TYPE_BOOL:
        setattr(msg, fd.name, True)
    elif fd.type in (fd.TYPE_DOUBLE, fd.TYPE_FLOAT):
        setattr(msg, fd.name, 1.5)
    else:
        setattr(msg, fd.name, 7)


def _attrs(n_bytes: int, prefix: str = "k") -> Dict[str, str]:
    out, size, j = {}, 0, 0
    while size < n_bytes:
        out[f"{prefix}{j:03d}"] = "v" * 200
        size += 212
        j += 1
    return out


def sparse_wide(envs: uc.Envs) -> Dict[str, tuple]:
    """The feature's target: a few fields of 64 present, the gaps between
    them far wider than an item's 256-byte pad."""
    full = _wide(envs, f01_string="s" * 1000)
    _set_number(full, 60)
    full.attrs.update(_attrs(10_000))
    only_attrs = _wide(envs)
    only_attrs.attrs.update(_attrs(10_000))
    only_first = _wide(envs, f01_string="s" * 1000)
    return {
        "sparse:f01+f60+attrs": ("bench.Wide64", full.SerializeToString()),
        "sparse:attrs-only": ("bench.Wide64", only_attrs.SerializeToString()),
        "sparse:f01-only": ("bench.Wide64", only_first.SerializeToString()),
    }


# ---- group 3: chunk joins ------------------------------------------------------

def chunk_joins(envs: uc.Envs) -> Dict[str, tuple]:
    """An ``items`` run and an ``attrs`` map of ~9 KB and ~13 KB (3-4 chunks
    each), the specials string starting at item-text offsets 4081..4100 so
    every one of its characters sits at, before and across the 4096-byte
    slice edge; every other field absent, so defaults on both sides."""
    out = {}
    for size in (9_000, 13_000):
        for at in range(SLICE - 15, SLICE + 5):
            m = _wide(envs)
            # item text `"items":[{"key":"` is 17 bytes, `"attrs":{"a":"` 14
            m.items.add(key="x" * (at - 17) + SPECIALS + "tail", value=at)
            for j in range((size - at) // 60):
                m.items.add(key=f"i{j}" + SPECIALS, value=j, weight=j / 4)
            m.attrs["a"] = "y" * (at - 14) + SPECIALS + "tail"
            m.attrs.update(_attrs(size - at, prefix="b"))
            out[f"join:{size}@{at}"] = ("bench.Wide64", m.SerializeToString())
    return out


# ---- group 4: hand-assembled top-level wires -----------------------------------

def _v(num: int, val: int = 1) -> bytes:
    return tag(num, 0) + pc.vi(val)


def _positions(name: str, piece: bytes, before: bytes, after: bytes):
    """``piece`` between two real fields, first, and last."""
    return {f"{name}:between": before + piece + after,
            f"{name}:first": piece + after,
            f"{name}:last": before + piece}


def hand_wires(envs: uc.Envs) -> Dict[str, tuple]:
    """Top-level wires holding what does not advance the classic walker's
    ``prev_number`` — an unknown field, a known field in a foreign wire type,
    an empty packed run, an empty run followed by a non-empty one — and
    out-of-order fields, each between two real fields, first, and last.

    x.Rich: s_string 14, s_enum 16, no field 39, ri (repeated int32) 40,
    tail 1000.  t.Sink: r_int64 3, r_int32 5, snake_case_field and custom
    (strings) near the end, no field 900."""
    out: Dict[str, tuple] = {}
    F = pc.F
    rich = {
        "unknown": _v(39),
        "foreign-wire-type": ld(16, b"abc"),
        "empty-packed": ld(40, b""),
        "empty-then-values": ld(40, b"") + ld(40, b"\x01\x02"),
        "out-of-order": _v(20) + _v(17),             # one_i 20, then opt_i32 17
    }
    for name, piece in rich.items():
        for cid, w in _positions(f"rich:{name}", piece, ld(14, b"str"),
                                 ld(1000, b"z")).items():
            out[cid] = ("x.Rich", w)
    sink = {
        "unknown": _v(900),
        "foreign-wire-type": _v(F["snake_case_field"]),
        "empty-packed": ld(F["r_int32"], b""),
        "empty-then-values": ld(F["r_int32"], b"") + ld(F["r_int32"], b"\x01\x02"),
        "out-of-order": ld(F["blob"], b"b") + _v(F["r_bool"]),
    }
    for name, piece in sink.items():
        for cid, w in _positions(f"sink:{name}", piece, _v(F["r_int64"], 5),
                                 ld(F["custom"], b"c")).items():
            out[cid] = ("t.Sink", w)
    return out


OUT_OF_ORDER = tuple(f"{m}:out-of-order:{p}" for m in ("rich", "sink")
                     for p in ("between", "first", "last"))


# ---- group 5: a top-level Any ---------------------------------------------------

def any_tops(envs: uc.Envs) -> Dict[str, tuple]:
    """t.Holder whose only top-level field is an Any: a plain payload (its
    defaults follow "@type") and a Timestamp payload."""
    leaf = ld(1, (ac.TG + "t.Leaf").encode()) + ld(2, ld(2, b"x"))
    ts = (ld(1, (ac.TG + "google.protobuf.Timestamp").encode())
          + ld(2, tag(1, 0) + pc.vi(1_700_000_000)))
    return {"any:plain": ("t.Holder", ld(1, leaf)),
            "any:timestamp": ("t.Holder", ld(1, ts))}


GROUPS = {
    "corpus": corpus,
    "sparse": sparse_wide,
    "joins": chunk_joins,
    "hand": hand_wires,
    "any": any_tops,
}


def all_cases(envs: uc.Envs) -> Dict[str, tuple]:
    out: Dict[str, tuple] = {}
    for fn in GROUPS.values():
        out.update(fn(envs))
    return out


# ---- runner ----------------------------------------------------------------------

def run(envs: uc.Envs, cases: Dict[str, tuple], flags: int
        ) -> Dict[str, Tuple[int, bytes, int, int]]:
    """case id -> (status, envelope bytes | None, pad, request id), one
    envelope batch of at most BATCH slots per schema.  ``uc.run_envelopes``
    with the slot's ``pad`` (the decode path tag) kept."""
    res: Dict[str, Tuple[int, bytes, int, int]] = {}
    by_schema: Dict[str, List[str]] = {}
    for cid, (name, _) in cases.items():
        by_schema.setdefault(name, []).append(cid)
    for name, ids in by_schema.items():
        s = envs.schema(name)
        tool = tool_for(envs, name)
        for part in pc._chunks(ids, BATCH):
            wires = [cases[c][1] for c in part]
            enc, _ = s.engine.encode_batch(
                uc.envelope_bodies(tool, list(range(len(part)))), mode=0)
            assert all(int(r["status"]) == 0 for r in enc)
            dec, outs = s.engine.decode_batch(wires, [s.idx] * len(part),
                                              mode=0 | flags)
            for k, (cid, r, o) in enumerate(zip(part, dec, outs)):
                res[cid] = (int(r["status"]), o, int(r["pad"]), k)
    return res


def raw_slice(out: bytes) -> bytes:
    """The structuredContent value of a structured envelope."""
    at = out.rfind(uc.P_STRUCT)
    return out[at + len(uc.P_STRUCT):len(out) - len(uc.P_TAIL)]


def compare(cases: Dict[str, tuple], classic, coop, flags: int,
            ids: Sequence[str] = ()) -> List[str]:
    """Every difference between two runs' answers (the classic kernel's
    first, the one under test second), and every envelope defect of the
    second."""
    bad = []
    for cid in (ids or cases):
        st, out, _, _ = classic[cid]
        wst, wout, wpad, k = coop[cid]
        if (st, out) != (wst, wout):
            a, b = out or b"", wout or b""
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y),
                      min(len(a), len(b)))
            bad.append(f"{cid} flags {flags}: first {st}, second {wst}, "
                       f"bytes differ at {at}: {a[max(at - 60, 0):at + 60]!r} "
                       f"!= {b[max(at - 60, 0):at + 60]!r}")
        elif wst == 0 and flags & uc.DM_STRUCTURED:
            why = uc.check_envelope(wout, uc.id_token(k))
            if why:
                bad.append(f"{cid}: {why}")
    return bad
