"""Hand-assembled out-of-order and re-occurring wires for DM_REORDER
(``test_reorder_host.py`` on the CPU build, ``test_gpu_reorder.py`` on gfx950).

``CASES``: case id -> (schema name, wire, expect).  "ok" = status 0, ``pad`` 3
and the oracle's value (``json_format`` over ``FromString`` of the same wire,
by ``unpopulated_corpus.verdict``); "keep" = the pass gives up, the slot stays
E_UNSUPPORTED, ``pad`` untouched; "refused" = status stays non-zero.  Schemas:
those of the existing corpora, and proto2 ``g.G`` for a group field.
"""

import json
from typing import Dict, NamedTuple

from google.protobuf import descriptor_pb2, message_factory

import any_corpus as ac
import protojson_corpus as pc
import unpopulated_corpus as uc
import wg_flags_corpus as wc
from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos
from protojson_corpus import ld, tag, vi

DM_REORDER = RO = 16
# every kind, and both flags on the envelope and the bare kind
MODES = [0 | RO, 1 | RO, 2 | RO, 0 | RO | uc.DM_UNPOPULATED | uc.DM_STRUCTURED,
         1 | RO | uc.DM_UNPOPULATED]
RO_MAX_RUNS = 256      # common.h
BIG = 17_000           # a slot past WG_DEC_MIN_BYTES


def v(num: int, val: int = 1) -> bytes:
    return tag(num, 0) + vi(val)


def group_fdp():
    """proto2 g.G { optional group Inner = 1 { int32 x = 2 }; int32 a = 3, b = 4 }"""
    fdp = descriptor_pb2.FileDescriptorProto(name="g/g.proto", package="g",
                                             syntax="proto2")
    m = fdp.message_type.add(name="G")
    m.nested_type.add(name="Inner").field.add(name="x", number=2, type=5, label=1)
    m.field.add(name="inner", number=1, type=10, label=1, type_name=".g.G.Inner")
    m.field.add(name="a", number=3, type=5, label=1)
    m.field.add(name="b", number=4, type=5, label=1)
    svc = fdp.service.add(name="GService")
    svc.method.add(name="Echo", input_type=".g.G", output_type=".g.G")
    return fdp


class Envs(NamedTuple):
    base: uc.Envs
    group: uc.Schema
    group_tool: str

    def schema(self, name: str) -> uc.Schema:
        return self.group if name == "g.G" else self.base.schema(name)

    def tool(self, name: str) -> str:
        return self.group_tool if name == "g.G" else wc.tool_for(self.base, name)


def make_envs(engine_factory) -> Envs:
    pool = build_pool([group_fdp()])
    infos = {m.tool_name(): m for m in
             extract_method_infos([group_fdp()], pool, compat_names=False)}
    eng = engine_factory(infos)
    cls = message_factory.GetMessageClass(pool.FindMessageTypeByName("g.G"))
    return Envs(uc.make_envs(engine_factory),
                uc.Schema(eng, pool, cls, eng.tables.msg_index["g.G"]),
                sorted(infos)[0])


def _runs(n: int) -> bytes:   # x.Rich: ri (40) and leaves (22) interleaved
    return b"".join(v(40, i) if i % 2 == 0 else ld(22, b"") for i in range(n))


def _cases() -> Dict[str, tuple]:
    R, H, N = "x.Rich", "t.Holder", "complex.NodeRequest"
    leaf_url = ld(1, (ac.TG + "t.Leaf").encode())
    unknowns = (v(4) + v(500) + tag(501, 3) + v(1) + tag(501, 4)   # unknown group
                + ld(5, b"abc") + v(3, 7))                         # foreign wire type
    return {
        "swap-top": (R, v(4) + v(3), "ok"),
        "swap-depth2": (R, ld(14, b"s") + ld(21, ld(2, b"t") + v(1, 5)), "ok"),
        "swap-in-repeated": (R, ld(22, ld(2, b"t") + v(1, 5)) + ld(22, v(1)), "ok"),
        "swap-in-map-value": (R, ld(23, ld(1, b"k") + ld(2, ld(2, b"t") + v(1, 5))),
                              "ok"),
        "scalar-twice": (R, v(3, 1) + v(4, 9) + v(3, 2), "ok"),
        "string-twice": (R, ld(14, b"a") + v(3) + ld(14, b"b"), "ok"),
        "repeated-scalar-3-runs": (R, ld(40, b"\x01\x02") + v(3) + v(40, 3) + v(4)
                                   + ld(40, b"\x04"), "ok"),
        "repeated-message-split": (R, ld(22, v(1)) + v(3) + ld(22, v(1, 2))
                                   + ld(22, b"") + v(4) + ld(22, ld(2, b"z")), "ok"),
        "message-merge": (R, ld(21, ld(2, b"a") + v(1)) + v(3)
                          + ld(21, v(1, 2) + ld(2, b"b") + v(1, 3)), "ok"),
        "message-127-128": (R, ld(21, ld(2, b"x" * 123) + v(1))
                            + ld(21, ld(2, b"y" * 124) + v(1, 2)), "ok"),
        "oneof-X-Y": (R, ld(19, b"x") + v(20, 5) + v(3), "ok"),
        "oneof-X1-Y-X2": (R, ld(19, b"x") + v(20, 5) + ld(19, b"z") + v(3), "ok"),
        "oneof-message-X1-X2": (H, ld(5, leaf_url) + ld(4, b"z")
                                + ld(5, ld(2, ld(2, b"t"))), "ok"),
        "oneof-legacy-go": (R, ld(1000, b"z") + v(20, 5), "ok"),
        "any-value-before-url": (H, ld(4, b"z") + ld(1, ld(2, v(1, 7)) + leaf_url),
                                 "ok"),
        "map-split": (R, ld(24, ld(1, b"a") + v(2, 1)) + v(3)
                      + ld(24, v(2, 2) + ld(1, b"b"))
                      + ld(24, ld(1, b"c") + ld(1, b"d") + v(2, 3)), "ok"),
        "unknowns": (R, unknowns, "ok"),
        "unknowns-big": (R, ld(1000, b"z" * BIG) + unknowns, "ok"),
        "runs-64": (R, _runs(64), "ok"),
        "runs-65": (R, _runs(65), "ok"),
        "runs-max": (R, _runs(RO_MAX_RUNS), "ok"),
        "runs-max+1": (R, _runs(RO_MAX_RUNS + 1), "keep"),
        "depth-max": (N, v(2, 3) + ld(1, uc._node(uc.MAX_RECURSE - 1)), "ok"),
        "depth-max+1": (N, v(2, 3) + ld(1, uc._node(uc.MAX_RECURSE)), "keep"),
        "truncated": (R, v(4) + v(3) + ld(14, b"abc")[:-1], "refused"),
        "known-group": ("g.G", v(4) + tag(1, 3) + v(2, 5) + tag(1, 4) + v(3), "keep"),
    }


CASES = _cases()


def run(envs: Envs, ids, mode: int) -> Dict[str, tuple]:
    """case id -> (status, bytes | None, pad, request id), one batch per schema."""
    res: Dict[str, tuple] = {}
    for name in sorted({CASES[c][0] for c in ids}):
        part = [c for c in ids if CASES[c][0] == name]
        s = envs.schema(name)
        if mode & 3 == 0:
            enc, _ = s.engine.encode_batch(
                uc.envelope_bodies(envs.tool(name), list(range(len(part)))), mode=0)
            assert all(int(r["status"]) == 0 for r in enc)
        dec, outs = s.engine.decode_batch([CASES[c][1] for c in part],
                                          [s.idx] * len(part), mode=mode)
        for k, (cid, r, o) in enumerate(zip(part, dec, outs)):
            res[cid] = (int(r["status"]), o, int(r["pad"]), k)
    return res


def judge(envs: Envs, cid: str, mode: int, got: tuple):
    """None, or what is wrong with one answer."""
    name, wire, expect = CASES[cid]
    status, out, pad, k = got
    if expect == "keep":
        ok = status == pc.E_UNSUPPORTED and pad in (0, 2)
        return None if ok else f"gave-up slot changed: status {status} pad {pad}"
    if expect == "refused":
        return None if status != 0 else f"printed {out!r}"
    if (status, pad) != (0, 3):
        return f"status {status} pad {pad}"
    kind = mode & 3
    if kind == 0 and mode & uc.DM_STRUCTURED:
        why = uc.check_envelope(out, uc.id_token(k))
        if why:
            return why
        out = wc.raw_slice(out)
    elif kind == 0:
        out = json.loads(out)["result"]["content"][0]["text"].encode()
    elif kind == 2:
        out = json.loads(out)["text"].encode()
    unpop = bool(mode & uc.DM_UNPOPULATED) and kind != 2
    return uc.verdict(envs.schema(name), wire, status, out, unpop)
