"""Wide-schema corpus: messages past the encode walker's bit-set widths
(64 fields / 32 oneofs before this corpus existed, 128 / 64 now) and field
numbers with 3- to 5-byte tags.

A plain helper module in the style of ``protojson_corpus.py``, whose
``_verdict`` contract and ``same_json`` comparison it imports: where the
oracle (``google.protobuf.json_format`` on the real message classes) raises
the kernel status is non-zero; where it accepts the kernel returns status 0
and an equal value, unless the case carries a ``HOST`` tag quoting a rule of
docs/KERNELS.md.

Three messages, each the input and output of an ``Echo`` method:

* ``w.Wide``   — 131 fields numbered 1..131 (sorted index = number - 1): 130
  ``f_NNN`` fields cycling through eleven kinds plus ``child`` (``w.Wide``
  itself, index 40: the bit sets are per frame);
* ``w.Oneofs`` — 66 real oneofs ``oNN {int32 a_NN, string b_NN}`` at field
  indices 2*NN and 2*NN+1, then three proto3 ``optional`` fields whose
  synthetic oneofs come last and take no oneof bit;
* ``w.Sparse`` — field numbers at both sides of every tag-length step.
"""

from __future__ import annotations

import json
from typing import Any, Dict, List, NamedTuple, Optional, Sequence

from google.protobuf import json_format, message_factory
from google.protobuf.message import DecodeError

import protojson_corpus as pc
from protojson_corpus import _verdict, same_json  # noqa: F401  (the contract)
from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos
from ggrmcp_amd.utils.protobuild import FileBuilder

DM_UNPOPULATED = 4
HOST_STATUSES = pc.HOST_STATUSES
HOST_CAP = pc.HOST_CAP

# the KERNELS.md rules this corpus' HOST tags quote
LIMIT = ("a member at field index 128 or above, or of a oneof with index 64 "
         "or above, takes the host path")
FILL = "defaults that outgrow the slot end in E_OVERFLOW"

# ---- schemas ----------------------------------------------------------------

KINDS = ["int32", "string", "int64", "bool", "double", "bytes", "enum", "leaf",
         "packed", "rstring", "map"]
KIND_SHIFT = 3          # index 64 is an int32, 65 a string, 126 a Leaf, ...
CHILD_INDEX = 40
N_WIDE = 131            # 130 cycling fields + child
N_ONEOFS = 66
SPARSE_NUMBERS = [1, 15, 16, 2047, 2048, 262143, 262144, 33554431, 33554432,
                  536870911]
SPARSE_KINDS = ["int32", "string", "rstring", "map", "leaf", "int64", "rleaf",
                "bool", "double", "string"]
MAX_FIELD = 536870911   # 2^29 - 1

# the indices the cases visit: both sides of every word of the bit sets
EDGE = [0, 31, 32, 62, 63, 64, 65, 66, 126, 127, 128, 129]


def wide_kind(index: int) -> str:
    if index == CHILD_INDEX:
        return "child"
    k = index if index < CHILD_INDEX else index - 1
    return KINDS[(k + KIND_SHIFT) % len(KINDS)]


def wide_name(index: int) -> str:
    return "child" if index == CHILD_INDEX else f"f_{index + 1:03d}"


def json_name(proto_name: str) -> str:
    return pc._camel(proto_name)


def _add_field(m, name: str, number: int, kind: str) -> None:
    if kind == "enum":
        m.field(name, number, "enum", enum="Color")
    elif kind == "leaf":
        m.field(name, number, "message", message="Leaf")
    elif kind == "rleaf":
        m.field(name, number, "message", message="Leaf", repeated=True)
    elif kind == "child":
        m.field(name, number, "message", message="Wide")
    elif kind == "packed":
        m.field(name, number, "int32", repeated=True)
    elif kind == "rstring":
        m.field(name, number, "string", repeated=True)
    elif kind == "map":
        m.map_field(name, number, "string", "int32")
    else:
        m.field(name, number, kind)


def wide_fdp():
    fb = FileBuilder("w/wide.proto", "w")
    fb.enum("Color", [("C_ZERO", 0), ("C_ONE", 1), ("C_NEG", -1)])
    fb.message("Leaf").field("id", 1, "int32").field(
        "tag", MAX_FIELD, "string").done()
    m = fb.message("Wide")
    for i in range(N_WIDE):
        _add_field(m, wide_name(i), i + 1, wide_kind(i))
    m.done()
    m = fb.message("Oneofs")
    for o in range(N_ONEOFS):
        m.field(f"a_{o:02d}", 2 * o + 1, "int32", oneof=f"o{o:02d}")
        m.field(f"b_{o:02d}", 2 * o + 2, "string", oneof=f"o{o:02d}")
    m.field("opt_i", 2 * N_ONEOFS + 1, "int32", optional=True)
    m.field("opt_s", 2 * N_ONEOFS + 2, "string", optional=True)
    m.field("opt_b", 2 * N_ONEOFS + 3, "bool", optional=True)
    m.done()
    m = fb.message("Sparse")
    for n, (num, kind) in enumerate(zip(SPARSE_NUMBERS, SPARSE_KINDS)):
        _add_field(m, f"s_{n}", num, kind)
    m.done()
    for name in ("Wide", "Oneofs", "Sparse"):
        fb.service(f"{name}Service").method("Echo", name, name).done()
    return fb.build()


MESSAGES = ("w.Wide", "w.Oneofs", "w.Sparse")


class Env(NamedTuple):
    engine: Any
    pool: Any
    infos: Any
    cls: Dict[str, Any]    # message full name -> class
    idx: Dict[str, int]    # message full name -> table index
    tool: Dict[str, str]   # message full name -> its Echo tool


def make_env(engine_factory) -> Env:
    fdps = [wide_fdp()]
    pool = build_pool(fdps)
    infos = {m.tool_name(): m
             for m in extract_method_infos(fdps, pool, compat_names=False)}
    engine = engine_factory(infos)
    return Env(
        engine, pool, infos,
        {n: message_factory.GetMessageClass(pool.FindMessageTypeByName(n))
         for n in MESSAGES},
        {n: engine.tables.msg_index[n] for n in MESSAGES},
        {n: next(t for t, mi in infos.items()
                 if mi.input_descriptor.full_name == n) for n in MESSAGES})


# ---- cases ------------------------------------------------------------------

class Case(NamedTuple):
    id: str
    msg: str               # message full name
    data: Any              # JSON text (ACCEPT/REJECT) or wire bytes (WIRES)
    host: Optional[str] = None


_j = pc._j

_VALUES = {
    "int32": (-7, 9), "string": ("é\"x", "y"), "int64": ("-9007199254740993", "4"),
    "bool": (True, False), "double": (1.5, -2.25), "bytes": ("AAEC", "/w=="),
    "enum": ("C_NEG", "C_ONE"), "leaf": ({"id": 3, "tag": "t"}, {"id": 4}),
    "packed": ([1, -2, 300], [5]), "rstring": (["a", "", "b"], ["c"]),
    "map": ({"k": 1, "": -2}, {"z": 3}), "child": ({}, {}),
    "rleaf": ([{"id": 1}, {}, {"tag": "x"}], [{}]),
}


def _val(kind: str, second: bool = False) -> str:
    return _j(_VALUES[kind][1 if second else 0])


def _member(name: str, kind: str, second: bool = False) -> str:
    return f"{_j(name)}:{_val(kind, second)}"


def _wide_jname(i: int) -> str:
    return json_name(wide_name(i))


def _host(i: int) -> Optional[str]:
    return LIMIT if i >= 128 else None


def _first_index(kind: str, lo: int, hi: int) -> int:
    return next(i for i in range(lo, hi) if wide_kind(i) == kind)


def _accept_cases() -> List[Case]:
    c: List[Case] = []
    add = lambda i, m, d, host=None: c.append(Case(i, m, d, host))  # noqa: E731
    W, O, S = MESSAGES
    for i in EDGE:
        k = wide_kind(i)
        add(f"alone-{i}-{k}", W, "{%s}" % _member(_wide_jname(i), k), _host(i))
    for i in EDGE:
        if i < 128:
            k = wide_kind(i)
            add(f"child-alone-{i}-{k}", W,
                '{"child":{%s}}' % _member(_wide_jname(i), k))
    add("proto-name-64", W, "{%s}" % _member(wide_name(64), wide_kind(64)))
    add("all-below-128", W, "{%s}" % ",".join(
        _member(_wide_jname(i), wide_kind(i)) for i in range(128)))
    add("all-below-128-no-child", W, "{%s}" % ",".join(
        _member(_wide_jname(i), wide_kind(i)) for i in range(128)
        if i != CHILD_INDEX))
    # the same member in parent and child: the bit sets are per frame
    add("same-index-parent-and-child", W,
        '{"f065":1,"child":{"f065":2,"child":{"f065":3}},"f127":{"id":1}}')
    for a, b in [(i, i + 32) for i in range(8)] + [(31, 63)]:
        add(f"oneof-pair-{a}-{b}", O, _j({f"a{a:02d}": a + 1, f"b{b:02d}": "s"}))
    add("oneofs-0-63-a", O, _j({f"a{o:02d}": o for o in range(64)}))
    add("oneofs-0-63-b", O, _j({f"b{o:02d}": f"v{o}" for o in range(64)}))
    add("oneof-64-alone", O, '{"a64":5}', LIMIT)
    add("oneof-65-alone", O, '{"b65":"x"}', LIMIT)
    # index 132..134, so under the same rule; their synthetic oneofs are
    # indices 66..68 of the message and must not be compiled as oneofs at all
    add("optional-zero", O, '{"optI":0,"optS":"","optB":false}', LIMIT)
    full = {}
    for n, kind in enumerate(SPARSE_KINDS):
        full[f"s{n}"] = _VALUES[kind][0]
        add(f"sparse-alone-{SPARSE_NUMBERS[n]}", S, _j({f"s{n}": _VALUES[kind][0]}))
    add("sparse-full", S, _j(full))
    add("sparse-empty", S, "{}")
    add("sparse-empty-nested", S, '{"s4":{},"s6":[{},{}],"s3":{},"s2":[]}')
    add("sparse-leaf-tag-only", S, '{"s4":{"tag":"t"},"s6":[{"tag":""},{"tag":"u"}]}')
    return c


def _reject_cases() -> List[Case]:
    c: List[Case] = []
    add = lambda i, m, d: c.append(Case(i, m, d))  # noqa: E731
    W, O, _S = MESSAGES
    for i in EDGE:
        k, jn = wide_kind(i), _wide_jname(i)
        same = "%s,%s" % (_member(jn, k), _member(jn, k, True))
        add(f"dup-{i}-{k}", W, "{%s}" % same)
        add(f"child-dup-{i}-{k}", W, '{"child":{%s}}' % same)
    for o in (0, 31, 32, 33, 63):
        add(f"oneof-both-{o}", O, _j({f"a{o:02d}": 1, f"b{o:02d}": "x"}))
        add(f"oneof-both-{o}-reversed", O, _j({f"b{o:02d}": "x", f"a{o:02d}": 1}))
    for kind in ("packed", "rstring", "map"):
        i = _first_index(kind, 67, 126)
        jn = _wide_jname(i)
        add(f"dup-{kind}-{i}", W, "{%s,%s}" % (_member(jn, kind),
                                             _member(jn, kind, True)))
        add(f"dup-{kind}-{i}-apart", W, "{%s,%s,%s}" % (
            _member(jn, kind), _member("f001", wide_kind(0)),
            _member(jn, kind, True)))
    return c


def _dup_names_cases() -> List[Case]:
    """One member under both of its names (proto name, then JSON name).  Go
    protojson keys its duplicate check by field number and refuses; Python's
    json_format keys it by spelling and lets the pair through (last one wins,
    repeated ones merge).  The kernels follow Go, so as for
    ``protojson_corpus.GO_STRICT`` only their refusal is asserted."""
    c: List[Case] = []
    W = MESSAGES[0]
    for i in EDGE:
        k = wide_kind(i)
        mixed = "%s,%s" % (_member(wide_name(i), k), _member(_wide_jname(i), k, True))
        c.append(Case(f"dup-names-{i}-{k}", W, "{%s}" % mixed))
        c.append(Case(f"child-dup-names-{i}-{k}", W, '{"child":{%s}}' % mixed))
    return c


def _five_byte_tag(field: int, wt: int) -> bytes:
    """The tag as a non-minimal 5-byte varint."""
    v = field << 3 | wt
    return bytes([(v >> (7 * k)) & 0x7F | (0x80 if k < 4 else 0)
                  for k in range(5)])


def _wire_cases() -> List[Case]:
    c: List[Case] = []
    S = MESSAGES[2]
    add = lambda i, d, host=None: c.append(Case(i, S, d, host))  # noqa: E731
    vi, tag, ld = pc.vi, pc.tag, pc.ld
    n = dict(zip(("i32", "str", "rstr", "map", "leaf", "i64", "rleaf", "bool",
                  "dbl", "last"), SPARSE_NUMBERS))
    add("tag5-int32", _five_byte_tag(n["i32"], 0) + vi(7))
    add("tag5-string", _five_byte_tag(n["str"], 2) + vi(2) + b"ab")
    add("tag5-in-leaf", ld(n["leaf"], _five_byte_tag(1, 0) + vi(3)))
    add("tag5-every-field", _five_byte_tag(n["i32"], 0) + vi(1)
        + _five_byte_tag(n["rstr"], 2) + vi(1) + b"x"
        + _five_byte_tag(n["bool"], 0) + vi(1)
        + _five_byte_tag(n["last"], 2) + vi(1) + b"z")
    add("max-field-string", ld(n["last"], b"end"))
    add("leaf-max-field", ld(n["leaf"], tag(1, 0) + vi(2) + ld(MAX_FIELD, b"t")))
    # field number 2^29: one past the legal range (2^29 - 1 is the last)
    add("field-2^29-varint", tag(1 << 29, 0) + vi(1))
    add("field-2^29-len", tag(n["i32"], 0) + vi(1) + ld(1 << 29, b"ab"))
    add("field-2^29-in-leaf", ld(n["leaf"], tag(1 << 29, 0) + vi(1)))
    add("field-2^32-tag-wraps", vi((1 << 35) | (1 << 3)) + vi(1))
    # unknown numbers between the known ones, every tag length
    add("unknown-between", tag(n["i32"], 0) + vi(1) + tag(17, 0) + vi(2)
        + tag(2049, 0) + vi(3) + tag(262145, 0) + vi(4) + tag(33554433, 0) + vi(5)
        + ld(n["last"], b"z"))
    return c


ACCEPT = _accept_cases()
REJECT = _reject_cases()
GO_STRICT = _dup_names_cases()
HAND_WIRES = _wire_cases()

# the hand-assembled wires json_format refuses (pinned, as in protojson_corpus)
WIRES_ORACLE_REJECTS = frozenset("""
    field-2^29-varint field-2^29-len field-2^29-in-leaf field-2^32-tag-wraps
""".split())


# ---- oracle + runners -------------------------------------------------------

def oracle_parse(env: Env, case: Case):
    return pc.oracle_parse(env.cls[case.msg], case.data)


def oracle_print(env: Env, msg: str, wire: bytes, flags: int = 0) -> Optional[str]:
    try:
        m = env.cls[msg].FromString(wire)
        return json_format.MessageToJson(
            m, indent=None, ensure_ascii=False,
            always_print_fields_with_no_presence=bool(flags & DM_UNPOPULATED))
    except (DecodeError, json_format.SerializeToJsonError):
        return None


# With DM_UNPOPULATED a w.Wide body prints ~1.5 KB of defaults (all 131:
# 1535 bytes).  A slot's scratch is 8 x wire + 1024 bytes, and in the
# workgroup kernel a nested message prints inside its item's 8 x wire + 256,
# so every SMALL w.Wide wire ends in E_OVERFLOW: the FILL rule, not a finding.
# The flag's list therefore keeps the one w.Wide wire large enough to print on
# both paths and four that are not, tagged; w.Oneofs and w.Sparse stay whole.
UNPOP_WIDE = {
    "all-below-128-no-child": None,
    "all-below-128": FILL,            # child {} prints 131 defaults in an item
    "alone-64-int32": FILL,
    "alone-129-map": FILL,
    "child-alone-64-int32": FILL,
}


def wires(env: Env, flags: int = 0) -> List[Case]:
    """WIRES: the oracle's serialization of every ACCEPT case (an encode-side
    HOST tag does not carry over: decode has no index limit), then the
    hand-assembled ones.  With DM_UNPOPULATED: see UNPOP_WIDE."""
    out = []
    for c in ACCEPT:
        host = None
        if flags & DM_UNPOPULATED and c.msg == MESSAGES[0]:
            if c.id not in UNPOP_WIDE:
                continue
            host = UNPOP_WIDE[c.id]
        out.append(Case(c.id, c.msg, oracle_parse(env, c).SerializeToString(),
                        host))
    return out + HAND_WIRES


def envelope(tool: str, text: str, rid: int) -> bytes:
    """``text`` verbatim as the arguments of a tools/call (json.dumps of a
    parsed object would drop the duplicate members the cases are about)."""
    return ('{"jsonrpc":"2.0","id":%d,"method":"tools/call","params":'
            '{"name":"%s","arguments":%s}}' % (rid, tool, text)).encode()


def encode_direct(env: Env, cases: Sequence[Case]):
    return env.engine.encode_batch(
        [c.data.encode() for c in cases], mode=1,
        msg_indices=[env.idx[c.msg] for c in cases], enforce=False)


def encode_envelope(env: Env, cases: Sequence[Case]):
    return env.engine.encode_batch(
        [envelope(env.tool[c.msg], c.data, i) for i, c in enumerate(cases)],
        mode=0)


def run_encode(env: Env, cases: Sequence[Case], encode=encode_direct) -> dict:
    """One encode batch over ``cases``; case id -> None | failure text."""
    enc, pbs = encode(env, cases)
    return pc.encode_verdicts(cases, [env.cls[c.msg] for c in cases], enc, pbs)


def run_decode(env: Env, cases: Sequence[Case], flags: int = 0,
               wg: Optional[bool] = None):
    """One mode-0 decode batch; returns (case id -> None | failure text,
    [(status, bytes)]).  ``wg`` is passed on where the engine takes it (the
    CPU build); the device routes by GGRMCP_WG_DEC_MIN alone."""
    n = len(cases)
    enc, _ = env.engine.encode_batch(
        [envelope(env.tool[c.msg], "{}", i) for i, c in enumerate(cases)], mode=0)
    assert all(int(r["status"]) == 0 for r in enc)
    kw = {} if wg is None else {"wg": wg}
    dec, outs = env.engine.decode_batch(
        [c.data for c in cases], [env.idx[c.msg] for c in cases], flags, **kw)
    res = {}
    for i, (c, r, o) in enumerate(zip(cases, dec, outs)):
        want = oracle_print(env, c.msg, c.data, flags)
        desc = env.cls[c.msg].DESCRIPTOR

        def equal(o=o, want=want, desc=desc, i=i):
            try:
                resp = json.loads(o)
                assert resp["result"]["isError"] is False
                text = resp["result"]["content"][0]["text"]
                g = pc.loads(text)
            except Exception as exc:
                return f"kernel text is not a result envelope: {exc!r} {o!r}"
            if resp["id"] != i:
                return f"envelope id {resp['id']} in slot {i}"
            if not same_json(g, pc.loads(want), desc):
                return f"\nkernel: {text!r}\noracle: {want!r}"
            dups = pc.duplicate_members(text)
            return f"duplicate JSON members {dups}: {text!r}" if dups else None

        res[c.id] = _verdict(c, int(r["status"]), want is not None, equal)
        if res[c.id]:
            res[c.id] += f"  wire={c.data.hex()[:200]}"
    raw = [(int(r["status"]), None if o is None else bytes(o))
           for r, o in zip(dec, outs)]
    return res, raw
