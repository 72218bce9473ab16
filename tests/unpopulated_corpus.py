"""Shared cases for the DM_UNPOPULATED / DM_STRUCTURED decode suites
(``test_unpopulated_surface.py`` and ``test_structured_envelope.py`` on the
CPU build, ``test_gpu_structured.py`` on gfx950).

A plain helper module, not a conftest.  It imports the protojson and Any
corpora read-only and adds a third schema set (hello, complex, ``x.Rich``,
proto2 ``x2.Old``, ``xw.Many``) for the targeted cases.

The oracle is ``json_format.MessageToDict(msg,
always_print_fields_with_no_presence=True, descriptor_pool=...)``.  Values
are compared parsed, never as bytes: the oracle appends unset fields after
the set ones, the kernel interleaves them by field number.
"""

from __future__ import annotations

import json
from typing import Any, Dict, List, NamedTuple, Optional, Sequence

from google.protobuf import json_format, message_factory

import any_corpus as ac
import protojson_corpus as pc
from examples.protos import ALL_FDPS
from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos
from ggrmcp_amd.utils.protobuild import FileBuilder
from protojson_corpus import ld, tag

DM_UNPOPULATED = 4
DM_STRUCTURED = 8
E_LIMIT = 5
MAX_RECURSE = 16   # common.h

SCALARS = pc.SCALAR_KINDS + ["string", "bytes"]


def rich_fdp():
    """x.Rich: one singular no-presence field of every kind, then presence,
    oneof, message, repeated and map fields — sparse numbers at the end so
    the gap fill's binary-search start is used too."""
    fb = FileBuilder("x/rich.proto", "x")
    fb.enum("Mode", [("MODE_ZERO", 0), ("MODE_ONE", 1)])
    fb.message("Leaf").field("id", 1, "int32").field("tag", 2, "string").done()
    m = fb.message("Rich")
    n = 0
    for k in SCALARS:
        n += 1
        m.field(f"s_{k}", n, k)
    m.field("s_enum", 16, "enum", enum="Mode")
    # the real oneof is declared first: synthetic (proto3 optional) oneofs
    # must come after every other oneof of the message
    m.field("one_s", 19, "string", oneof="k")
    m.field("one_i", 20, "int32", oneof="k")
    m.field("opt_i32", 17, "int32", optional=True)
    m.field("opt_str", 18, "string", optional=True)
    m.field("leaf", 21, "message", message="Leaf")
    m.field("leaves", 22, "message", message="Leaf", repeated=True)
    m.map_field("lm", 23, "string", "message", "Leaf")
    m.map_field("im", 24, "string", "int32")
    m.field("ri", 40, "int32", repeated=True)
    m.field("tail", 1000, "string")
    m.done()
    fb.service("RichService").method("Echo", "Rich", "Rich").done()
    return fb.build()


def old_fdp():
    """x2.Old, proto2: every singular field has presence, so only the
    repeated and map fields are ever filled in."""
    fb = FileBuilder("x2/old.proto", "x2", syntax="proto2")
    m = fb.message("Old")
    m.field("a", 1, "int32")
    m.field("r", 2, "int32", repeated=True)
    m.map_field("m", 3, "string", "int32")
    m.field("s", 4, "string")
    m.done()
    fb.service("OldService").method("Echo", "Old", "Old").done()
    return fb.build()


class Schema(NamedTuple):
    """One message type of one engine: what a run needs."""
    engine: Any
    pool: Any
    cls: Any
    idx: int


class Envs(NamedTuple):
    sink: pc.Env
    holder: ac.Env
    engine: Any     # third schema set
    pool: Any
    infos: Dict[str, Any]

    def schema(self, full_name: str) -> Schema:
        if full_name in ("t.Sink", "bench.Wide64", "bench.Inner"):
            e, pool = self.sink.engine, self.sink.pool
        elif full_name == "t.Holder":
            e, pool = self.holder.engine, self.holder.pool
        else:
            e, pool = self.engine, self.pool
        cls = message_factory.GetMessageClass(pool.FindMessageTypeByName(full_name))
        return Schema(e, pool, cls, e.tables.msg_index[full_name])


def make_envs(engine_factory) -> Envs:
    fdps = ALL_FDPS + [rich_fdp(), old_fdp(), wide_holder_fdp()]
    pool = build_pool(fdps)
    infos = {m.tool_name(): m
             for m in extract_method_infos(fdps, pool, compat_names=False)}
    return Envs(pc.make_env(engine_factory), ac.make_env(engine_factory),
                engine_factory(infos), pool, infos)


# ---- oracle + runner ----------------------------------------------------------

def oracle(s: Schema, wire: bytes, unpopulated: bool = True) -> Optional[dict]:
    """Parsed protojson of ``wire``, or None where the oracle refuses."""
    try:
        msg = s.cls.FromString(wire)
        return json_format.MessageToDict(
            msg, always_print_fields_with_no_presence=unpopulated,
            descriptor_pool=s.pool)
    except Exception:
        return None


def decode(s: Schema, wires: Sequence[bytes], flags: int):
    """One bare-JSON (mode 1) batch -> [(status, bytes|None)]."""
    res = []
    for part in pc._chunks(list(wires), pc.MAX_BATCH):
        dec, outs = s.engine.decode_batch(part, [s.idx] * len(part),
                                          mode=1 | flags)
        res += [(int(r["status"]), o) for r, o in zip(dec, outs)]
    return res


def verdict(s: Schema, wire: bytes, status: int, out: Optional[bytes],
            unpopulated: bool, dup_keys_ok: bool = False) -> Optional[str]:
    """None, "host" (left with E_UNSUPPORTED/E_OVERFLOW) or a failure text.
    ``dup_keys_ok``: the corpus's DUP_KEYS rule — wire that repeats a map
    key prints both members; nothing else may print a name twice."""
    want = oracle(s, wire, unpopulated)
    if want is None:
        return None if status != 0 else f"oracle refuses, kernel printed {out!r}"
    if status in pc.HOST_STATUSES:
        return "host"
    if status != 0:
        return f"oracle accepts, kernel status {status}"
    try:
        got = pc.loads(out.decode())
    except Exception as exc:
        return f"kernel text is not JSON: {exc!r} {out!r}"
    if not ac.same_json(got, want, s.cls.DESCRIPTOR, s.pool):
        return f"\nkernel: {out!r}\noracle: {json.dumps(want)}"
    dups = [] if dup_keys_ok else pc.duplicate_members(out.decode())
    return f"duplicate JSON members {dups}: {out!r}" if dups else None


def corpus_wires(envs: Envs) -> Dict[str, tuple]:
    """case id -> (schema name, wire): the oracle's serialisation of every
    ACCEPT payload of both corpora, plus their hand-written WIRES."""
    out: Dict[str, tuple] = {}
    for c, w in zip(pc.ACCEPT, pc.accept_wires(envs.sink)):
        out[f"sink:{c.id}"] = ("t.Sink", w)
    for c in pc.WIRES:
        out[f"sink-wire:{c.id}"] = ("t.Sink", c.data)
    for c, w in zip(ac.ACCEPT, ac.accept_wires(envs.holder)):
        out[f"holder:{c.id}"] = ("t.Holder", w)
    for c in ac.WIRES:
        out[f"holder-wire:{c.id}"] = ("t.Holder", c.data)
    return out


def corpus_ids() -> List[str]:
    """The ids of corpus_wires(), computable at collection time."""
    return ([f"sink:{c.id}" for c in pc.ACCEPT]
            + [f"sink-wire:{c.id}" for c in pc.WIRES]
            + [f"holder:{c.id}" for c in ac.ACCEPT]
            + [f"holder-wire:{c.id}" for c in ac.WIRES])


def run_corpus(envs: Envs) -> Dict[str, tuple]:
    """case id -> (verdict with the flag clear, verdict with it set)."""
    cases = corpus_wires(envs)
    res: Dict[str, tuple] = {}
    for name in ("t.Sink", "t.Holder"):
        s = envs.schema(name)
        ids = [i for i, (n, _) in cases.items() if n == name]
        wires = [cases[i][1] for i in ids]
        plain = decode(s, wires, 0)
        unpop = decode(s, wires, DM_UNPOPULATED)
        dup_ok = {f"sink-wire:{c.id}" for c in pc.WIRES if c.host == pc.DUP_KEYS}
        for i, w, (st0, o0), (st1, o1) in zip(ids, wires, plain, unpop):
            res[i] = (verdict(s, w, st0, o0, False, i in dup_ok),
                      verdict(s, w, st1, o1, True, i in dup_ok))
    return res


# ---- targeted cases -----------------------------------------------------------

def _zero_wire(kind: str, num: int) -> bytes:
    if kind in ("double", "fixed64", "sfixed64"):
        return tag(num, 1) + b"\x00" * 8
    if kind in ("float", "fixed32", "sfixed32"):
        return tag(num, 5) + b"\x00" * 4
    if kind in ("string", "bytes"):
        return ld(num, b"")
    return tag(num, 0) + b"\x00"


def _node(depth: int) -> bytes:
    """complex.Node nested ``depth`` levels through children (field 2)."""
    w = b""
    for _ in range(depth - 1):
        w = ld(2, w)
    return w


def sink_descriptor():
    """t.Sink's descriptor without an engine (for collection-time ids)."""
    from ggrmcp_amd.utils.synthetic import synthetic_fdp

    return build_pool([pc.sink_fdp(), synthetic_fdp()]).FindMessageTypeByName("t.Sink")


def targeted_cases(sink_desc) -> Dict[str, tuple]:
    """case id -> (schema name, wire, expected): expected is "ok" (status 0
    and equal to the oracle) or the status number the kernel must return."""
    c: Dict[str, tuple] = {}
    for name in ("hello.HelloResponse", "complex.UserProfile", "complex.Document",
                 "complex.NodeRequest", "bench.Wide64", "t.Sink", "t.Holder",
                 "x.Rich", "x2.Old"):
        c[f"empty:{name}"] = (name, b"", "ok")
    # t.Sink: one wire per field, holding only that field
    for fd in sink_desc.fields:
        if fd.message_type is not None:
            body = ld(fd.number, b"")            # empty element / entry / body
        elif fd.type in (fd.TYPE_STRING, fd.TYPE_BYTES):
            body = ld(fd.number, b"v")
        elif fd.type in (fd.TYPE_DOUBLE, fd.TYPE_FIXED64, fd.TYPE_SFIXED64):
            body = tag(fd.number, 1) + b"\x00" * 6 + b"\xf0\x3f"   # 1.0
        elif fd.type in (fd.TYPE_FLOAT, fd.TYPE_FIXED32, fd.TYPE_SFIXED32):
            body = tag(fd.number, 5) + b"\x00\x00\x80\x3f"          # 1.0f
        else:
            body = tag(fd.number, 0) + b"\x01"
        c[f"sink-only:{fd.name}"] = ("t.Sink", body, "ok")
    # x.Rich: explicit zeros, one field at a time and all at once
    every = b""
    for n, k in enumerate(SCALARS, 1):
        c[f"zero:{k}"] = ("x.Rich", _zero_wire(k, n), "ok")
        every += _zero_wire(k, n)
    c["zero:enum"] = ("x.Rich", tag(16, 0) + b"\x00", "ok")
    c["zero:all"] = ("x.Rich", every + tag(16, 0) + b"\x00", "ok")
    c["zero:tail-1000"] = ("x.Rich", ld(1000, b""), "ok")
    c["neg-zero-double"] = ("x.Rich", tag(1, 1) + b"\x00" * 7 + b"\x80", "ok")
    c["optional-zero"] = ("x.Rich", tag(17, 0) + b"\x00" + ld(18, b""), "ok")
    c["optional-absent"] = ("x.Rich", tag(3, 0) + b"\x07", "ok")
    c["oneof-unset"] = ("x.Rich", ld(15, b"b"), "ok")
    c["oneof-set-zero"] = ("x.Rich", tag(20, 0) + b"\x00", "ok")
    c["msg-empty-body"] = ("x.Rich", ld(21, b""), "ok")
    c["msg-absent"] = ("x.Rich", ld(14, b"s"), "ok")
    c["msg-partial"] = ("x.Rich", ld(21, ld(2, b"t")), "ok")
    c["repeated-3-empty"] = ("x.Rich", ld(22, b"") * 3, "ok")
    c["map-value-missing"] = ("x.Rich", ld(23, ld(1, b"k")) + ld(24, ld(1, b"k")),
                              "ok")
    c["map-key-missing"] = ("x.Rich", ld(23, ld(2, ld(1, b"\x05")))
                            + ld(24, tag(2, 0) + b"\x03"), "ok")
    c["map-entry-empty"] = ("x.Rich", ld(23, b"") + ld(24, b""), "ok")
    c["map-msg-value-empty"] = ("x.Rich", ld(23, ld(1, b"k") + ld(2, b"")), "ok")
    c["enum-absent"] = ("x.Rich", ld(14, b"s") + tag(17, 0) + b"\x01", "ok")
    c["packed-empty-run"] = ("x.Rich", ld(40, b""), "ok")
    c["packed-empty-then-values"] = ("x.Rich", ld(40, b"") + ld(40, b"\x01\x02"),
                                     "ok")
    c["unknown-field-in-gap"] = ("x.Rich", tag(3, 0) + b"\x01" + tag(500, 0)
                                 + b"\x01" + ld(1000, b"z"), "ok")
    c["wrong-wire-type-is-unknown"] = ("x.Rich", ld(3, b"abc") + tag(4, 0) + b"\x02",
                                       "ok")
    c["out-of-order"] = ("x.Rich", tag(4, 0) + b"\x01" + tag(3, 0) + b"\x01",
                         pc.E_UNSUPPORTED)
    # Any payloads (t.Holder): plain payload with an empty value, url only
    url = ld(1, (ac.TG + "t.Leaf").encode())
    c["any-empty-value"] = ("t.Holder", ld(1, url + ld(2, b"")), "ok")
    c["any-url-only"] = ("t.Holder", ld(1, url), "ok")
    c["any-partial-payload"] = ("t.Holder", ld(1, url + ld(2, ld(2, b"x"))), "ok")
    c["any-in-repeated"] = ("t.Holder", ld(2, url) + ld(2, b"") + ld(4, b"z"), "ok")
    # recursion: the deepest nesting the frame stack holds, and one more
    c["node-depth-max-1"] = ("complex.NodeRequest", ld(1, _node(MAX_RECURSE - 1)),
                             "ok")
    c["node-depth-max"] = ("complex.NodeRequest", ld(1, _node(MAX_RECURSE)), E_LIMIT)
    # proto2: only repeated and map fields are filled
    c["proto2-some"] = ("x2.Old", tag(1, 0) + b"\x00", "ok")
    c["proto2-repeated"] = ("x2.Old", tag(2, 0) + b"\x05", "ok")
    return c


def wide_holder_fdp():
    """xw.Many { repeated xw.Wide w = 1 }, Wide = 40 no-presence fields."""
    fb = FileBuilder("xw/many.proto", "xw")
    m = fb.message("Wide")
    for i in range(1, 41):
        m.field(f"field_number_{i:02d}", i, "int64" if i % 2 else "string")
    m.done()
    fb.message("Many").field("w", 1, "message", message="Wide", repeated=True).done()
    fb.service("ManyService").method("Echo", "Many", "Many").done()
    return fb.build()


def expansion_case() -> tuple:
    """200 two-byte empty elements of a wide message type: ~150 KB of
    defaults from 400 bytes of wire, far past the slot's scratch.  The result
    must be E_OVERFLOW or a correct value and nothing else."""
    return "xw.Many", ld(1, b"") * 200


# ---- structured envelope ------------------------------------------------------

ENV_LENGTHS = (0, 63, 64, 65, 255, 256, 257)
ENV_SPECIALS = ['"', "\\", "\n", "\x01", "é", "😀"]
ENV_IDS = [7, -1, 2**53, "abc", 'q"\\', "", None, "i" * 46]   # last: 48 bytes


def envelope_strings() -> List[str]:
    """'a'*L with one special character first, and one last."""
    out = [""]
    for n in ENV_LENGTHS:
        if n == 0:
            continue
        for sp in ENV_SPECIALS:
            out.append(sp + "a" * (n - 1))
            if n > 1:
                out.append("a" * (n - 1) + sp)
    return out


def id_token(rid) -> bytes:
    return json.dumps(rid, ensure_ascii=False).encode()


def envelope_bodies(tool: str, ids: Sequence[Any]) -> List[bytes]:
    """tools/call bodies that prime the engine's id slots; the id token is
    spliced in verbatim so the replayed bytes are known exactly."""
    out = []
    for rid in ids:
        out.append(b'{"jsonrpc":"2.0","id":' + id_token(rid)
                   + b',"method":"tools/call","params":{"name":'
                   + json.dumps(tool).encode() + b',"arguments":{}}}')
    return out


P_HEAD = b'{"jsonrpc":"2.0","id":'
P_TEXT = b',"result":{"content":[{"type":"text","text":"'
P_STRUCT = b'"}],"structuredContent":'
P_TAIL = b',"isError":false}}'


def check_envelope(out: bytes, rid_token: bytes) -> Optional[str]:
    """The structured envelope, byte for byte: fixed framing, the id
    replayed verbatim, key order of ``result``, and a text block that
    unescapes to exactly the raw structuredContent slice."""
    if not out.startswith(P_HEAD + rid_token + P_TEXT):
        return f"head/id: {out[:120]!r}"
    if not out.endswith(P_TAIL):
        return f"tail: {out[-60:]!r}"
    resp = json.loads(out)
    res = resp["result"]
    if list(res) != ["content", "structuredContent", "isError"]:
        return f"result key order {list(res)}"
    if res["isError"] is not False:
        return "isError"
    at = out.rfind(P_STRUCT)
    if at < 0:
        return "no structuredContent"
    raw = out[at + len(P_STRUCT):len(out) - len(P_TAIL)]
    text = res["content"][0]["text"]
    if text.encode() != raw:
        return f"text block differs from the raw slice: {text!r} vs {raw!r}"
    if json.loads(raw) != res["structuredContent"]:
        return "raw slice is not the structuredContent value"
    return None


def run_envelopes(s: Schema, tool: str, wires: Sequence[Optional[bytes]],
                  ids: Sequence[Any], flags: int,
                  skip: Optional[Sequence[bool]] = None):
    """Mode-0 batch with request ids primed by an envelope encode batch."""
    enc, _ = s.engine.encode_batch(envelope_bodies(tool, ids), mode=0)
    assert all(int(r["status"]) == 0 for r in enc), [int(r["status"]) for r in enc]
    dec, outs = s.engine.decode_batch(list(wires), [s.idx] * len(wires),
                                      mode=0 | flags, skip=skip)
    return [(int(r["status"]), o) for r, o in zip(dec, outs)]
