"""google.protobuf.Any corpus, on the pattern of protojson_corpus.py.

The oracle is ``google.protobuf.json_format`` WITH ``descriptor_pool=pool``:
the schema lives in a private pool, so the helpers of protojson_corpus.py
(which call the oracle without one) cannot resolve a type URL.  Same verdict
rule (``protojson_corpus._verdict``): where the oracle raises the kernel
status is non-zero; where it accepts the status is 0 and the value equal;
a ``HOST`` tag quoting a docs/KERNELS.md rule also allows status 6/7.

Nothing byte-compares ``Any.value`` or a whole wire against the oracle's
serialisation — the kernels write legal 3-byte non-minimal length slots
inside the payload.  Encode results are parsed with the message class and
printed through the oracle; both sides are then compared as protojson values
(``same_json`` below: an Any is compared under its payload's schema, doubles
by the rules of the existing corpus).

Schema: ``t/anyh.proto`` (Holder, Leaf, Orphan, Deep, AnyService) imports
``u/other.proto`` and the well-known-type files; ``v/stranger.proto`` is
never loaded, so ``v.Stranger`` must not resolve.  ``t.Orphan`` is referenced
by no field anywhere: only the type table knows it.
"""

from __future__ import annotations

import json
from typing import Any, List, NamedTuple, Optional, Sequence

from google.protobuf import json_format, message_factory

import protojson_corpus as pc
from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos
from ggrmcp_amd.utils.protobuild import FileBuilder
from protojson_corpus import Case, ld, tag, vi

# docs/KERNELS.md host-escape rules (quoted verbatim by the HOST tags)
ANY_FIRST = ("an Any object whose first member is not `@type`, or whose "
             "`@type` string has backslash escapes or is longer than 256 bytes")
ANY_PAYLOAD = "an Any whose payload type is Struct, Value, ListValue or Any itself"
ANY_WIRE = ("on decode, an Any whose wire is not `[type_url][value]` in that "
            "order, each at most once")

TG = "type.googleapis.com/"
LEAF = {"@type": TG + "t.Leaf", "id": 5, "tag": "x"}


def other_fdp():
    fb = FileBuilder("u/other.proto", "u")
    fb.message("Other").field("d", 1, "double", repeated=True).done()
    return fb.build()


def anyh_fdp():
    fb = FileBuilder("t/anyh.proto", "t")
    fb.add_dependency(
        "u/other.proto", "google/protobuf/any.proto",
        "google/protobuf/duration.proto", "google/protobuf/timestamp.proto",
        "google/protobuf/wrappers.proto", "google/protobuf/field_mask.proto",
        "google/protobuf/empty.proto", "google/protobuf/struct.proto")
    any_ = "google.protobuf.Any"
    h = fb.message("Holder")
    h.field("a", 1, "message", message=any_)
    h.field("ra", 2, "message", message=any_, repeated=True)
    h.map_field("ma", 3, "string", "message", any_)
    h.field("after", 4, "string")
    h.field("oa", 5, "message", message=any_, oneof="k")
    h.field("oi", 6, "int32", oneof="k")
    h.done()
    fb.message("Leaf").field("id", 1, "int32").field("tag", 2, "string").done()
    fb.message("Orphan").field("n", 1, "int64").done()
    d = fb.message("Deep")
    d.field("inner", 1, "message", message=any_)
    d.field("next", 2, "message", message="Deep")
    d.field("s", 3, "string")
    d.done()
    fb.service("AnyService").method("Echo", "Holder", "Holder").done()
    return fb.build()


def stranger_fdp():
    """Never added to the pool: v.Stranger must stay unresolvable."""
    fb = FileBuilder("v/stranger.proto", "v")
    fb.message("Stranger").field("x", 1, "int32").done()
    return fb.build()


class Env(NamedTuple):
    engine: Any
    pool: Any
    infos: Any
    cls: Any          # t.Holder
    idx: int
    leaf_idx: int
    tool: str


def make_infos():
    fdps = [other_fdp(), anyh_fdp()]
    pool = build_pool(fdps)
    infos = {m.tool_name(): m
             for m in extract_method_infos(fdps, pool, compat_names=False)}
    return pool, infos


def make_env(engine_factory) -> Env:
    pool, infos = make_infos()
    engine = engine_factory(infos)
    tool = next(iter(infos))
    return Env(
        engine, pool, infos,
        message_factory.GetMessageClass(pool.FindMessageTypeByName("t.Holder")),
        engine.tables.msg_index["t.Holder"],
        engine.tables.msg_index["t.Leaf"],
        tool,
    )


def _j(obj) -> str:
    return json.dumps(obj, ensure_ascii=False)


def padded_url(total: int, name: str = "t.Leaf") -> str:
    """``p/p/.../t.Leaf`` of exactly ``total`` bytes."""
    pre = total - len(name)
    return ("p/" * pre)[:pre - 1] + "/" + name


URL_LENGTHS = list(range(62, 67)) + list(range(254, 259))

# payloads that travel as {"@type":..., "value": X}
WKT_VALUES = [
    ("duration", "Duration", "1.5s"),
    ("timestamp", "Timestamp", "2024-01-02T03:04:05.006Z"),
    ("int64", "Int64Value", "-9007199254740993"),
    ("uint64", "UInt64Value", "18446744073709551615"),
    ("int32", "Int32Value", -3),
    ("uint32", "UInt32Value", 7),
    ("bool", "BoolValue", True),
    ("double", "DoubleValue", 2.5),
    ("float", "FloatValue", 0.5),
    ("string", "StringValue", 'hi "there"\n'),
    ("bytes", "BytesValue", "AQIDBA=="),
    ("fieldmask", "FieldMask", "a.b,fooBar"),
]


def _wkt(name: str, value) -> dict:
    return {"@type": TG + "google.protobuf." + name, "value": value}


def _accept_cases() -> List[Case]:
    c: List[Case] = []
    payloads = [
        ("leaf", LEAF),
        ("orphan", {"@type": TG + "t.Orphan", "n": "7"}),
        ("other", {"@type": TG + "u.Other", "d": [1.5, -2.25, 1e300, 0.1]}),
        ("urlonly", {"@type": TG + "t.Leaf"}),
        ("empty", {}),
        ("tag200", {"@type": TG + "t.Leaf", "id": 1, "tag": "y" * 200}),
    ]
    for name, p in payloads:
        c.append(Case(f"a-{name}", _j({"a": p})))
        c.append(Case(f"ra-{name}", _j({"ra": [p, LEAF, p]})))
        c.append(Case(f"ma-{name}", _j({"ma": {"k": p, "k2": LEAF}})))
        c.append(Case(f"oa-{name}", _j({"oa": p})))
    # the walker resumes at the right byte after an Any
    c.append(Case("after-a", _j({"a": LEAF, "after": "z"})))
    c.append(Case("after-ra", _j({"ra": [LEAF], "after": "z"})))
    c.append(Case("after-ma", _j({"ma": {"k": LEAF}, "after": "z"})))
    c.append(Case("after-urlonly", _j({"a": {"@type": "t.Leaf"}, "after": "z"})))
    c.append(Case("any-last", _j({"after": "z", "a": LEAF})))
    c.append(Case("all-fields", _j({"a": LEAF, "ra": [LEAF, {}], "ma": {"k": LEAF},
                                    "after": "z", "oa": LEAF})))
    deep = {"@type": "t.Deep", "s": "1", "inner": {
        "@type": "t.Deep", "s": "2", "inner": {
            "@type": "t.Deep", "s": "3", "inner": LEAF}}}
    c.append(Case("deep-3", _j({"a": deep})))
    c.append(Case("deep-next", _j({"a": {"@type": "t.Deep", "next": {
        "inner": LEAF, "s": "n", "next": {"inner": {}}}, "s": "top"}})))
    c.append(Case("holder-in-ra", _j({"ra": [
        {"@type": "t.Holder", "a": LEAF, "after": "q"}]})))
    c.append(Case("holder-in-ma-in-holder", _j({"ma": {"k": {
        "@type": "t.Holder", "ma": {"j": LEAF}, "oi": 3}}})))
    for i, url in enumerate(("t.Leaf", "x/y/t.Leaf", TG + "t.Leaf")):
        c.append(Case(f"url-spelling-{i}", _j({"a": {"@type": url, "id": 9}})))
    for n in URL_LENGTHS:
        c.append(Case(f"url-len-{n}",
                      _j({"a": {"@type": padded_url(n), "id": n, "tag": "t"},
                          "after": "z"}),
                      ANY_FIRST if n > 256 else None))
    for name, wkt, v in WKT_VALUES:
        c.append(Case(f"wkt-{name}", _j({"a": _wkt(wkt, v)})))
    c.append(Case("wkt-in-ra", _j({"ra": [_wkt("Duration", "-3s"), LEAF,
                                          _wkt("StringValue", "")]})))
    c.append(Case("wkt-in-ma", _j({"ma": {"d": _wkt("Timestamp",
                                                    "1970-01-01T00:00:00Z"),
                                          "m": _wkt("FieldMask", "")}})))
    c.append(Case("wkt-then-after", _j({"a": _wkt("Int64Value", "5"),
                                        "after": "z"})))
    c.append(Case("empty-msg-payload",
                  _j({"a": {"@type": TG + "google.protobuf.Empty"}})))
    # whitespace in every gap of the Any
    c.append(Case("ws-message",
                  '{ "a" : { "@type" : "t.Leaf" , "id" : 5 , "tag" : "x" } , '
                  '"after" : "z" }'))
    c.append(Case("ws-wkt",
                  '{"a":\n{\t"@type" :"google.protobuf.Duration" ,\n "value" '
                  ': "2s"\n }\n}'))
    c.append(Case("ws-urlonly", '{"a":{ "@type":"t.Leaf" }}'))
    c.append(Case("null-any", '{"a":null,"after":"z"}'))
    c.append(Case("unicode-tag", _j({"a": {"@type": "t.Leaf", "tag": "é中😀\"\\"}})))
    # ---- HOST-tagged shapes ----
    c.append(Case("host-type-second",
                  _j({"a": {"id": 5, "@type": TG + "t.Leaf"}}), ANY_FIRST))
    c.append(Case("host-type-escaped",
                  '{"a":{"@type":"type.googleapis.com\\/t.Leaf","id":5}}',
                  ANY_FIRST))
    c.append(Case("host-struct-payload",
                  _j({"a": _wkt("Struct", {"k": 1, "l": [True, None]})}),
                  ANY_PAYLOAD))
    c.append(Case("host-any-in-any", _j({"a": _wkt("Any", LEAF)}), ANY_PAYLOAD))
    c.append(Case("host-url-300",
                  _j({"a": {"@type": padded_url(300), "id": 1}}), ANY_FIRST))
    return c


def _reject_cases() -> List[Case]:
    return [
        Case("unknown-type", _j({"a": {"@type": TG + "t.Nope", "id": 1}})),
        Case("unloaded-stranger", _j({"a": {"@type": TG + "v.Stranger", "x": 1}})),
        Case("type-empty", _j({"a": {"@type": "", "id": 1}})),
        Case("type-not-string", '{"a":{"@type":5,"id":1}}'),
        Case("type-missing", _j({"a": {"id": 1}})),
        Case("type-duplicate",
             '{"a":{"@type":"t.Leaf","id":1,"@type":"t.Leaf"}}'),
        Case("unknown-member", _j({"a": {"@type": "t.Leaf", "nope": 1}})),
        Case("wrong-typed-member", _j({"a": {"@type": "t.Leaf", "id": "abc"}})),
        Case("wrong-typed-in-ra", _j({"ra": [LEAF, {"@type": "t.Leaf", "tag": 5}]})),
        Case("trailing-comma", '{"a":{"@type":"t.Leaf",}}'),
        Case("any-not-object", '{"a":"t.Leaf"}'),
        Case("unterminated", '{"a":{"@type":"t.Leaf","id":5'),
        Case("wkt-bad-value", _j({"a": _wkt("Duration", "soon")})),
        Case("wkt-wrapper-range", _j({"a": _wkt("Int32Value", 2**31)})),
    ]


def _oracle_decides_cases() -> List[Case]:
    """Shapes on which protojson implementations differ; the oracle's verdict
    is taken at run time, never hard-coded."""
    c = [Case(f"novalue-{wkt}", _j({"a": {"@type": TG + "google.protobuf." + wkt}}))
         for wkt in ("Duration", "Timestamp", "FieldMask", "Int64Value",
                     "StringValue", "BytesValue")]
    c.append(Case("empty-via-value", _j({"a": _wkt("Empty", {})})))
    return c


def ld3(field: int, body: bytes) -> bytes:
    """Length-delimited field with the kernels' 3-byte non-minimal length."""
    n = len(body)
    return tag(field, 2) + bytes([n & 0x7F | 0x80, (n >> 7) & 0x7F | 0x80,
                                  (n >> 14) & 0x7F]) + body


def _wire_cases() -> List[Case]:
    url = ld(1, (TG + "t.Leaf").encode())
    leaf = ld(2, tag(1, 0) + vi(5) + ld(2, b"x"))      # Any.value = Leaf{5,"x"}
    after = ld(4, b"z")
    dur_url = ld(1, (TG + "google.protobuf.Duration").encode())
    return [
        Case("canonical", ld(1, url + leaf) + after),
        Case("empty-any", ld(1, b"") + after),
        Case("url-only", ld(1, url) + after),
        Case("url-only-wkt", ld(1, dur_url) + after),
        Case("wkt-value", ld(1, dur_url + ld(2, tag(1, 0) + vi(3))) + after),
        Case("empty-value", ld(1, url + ld(2, b"")) + after),
        Case("nonminimal-lengths",
             ld3(1, url + ld3(2, tag(1, 0) + vi(5) + ld3(2, b"x"))) + after),
        Case("in-ra-and-ma", ld(2, url + leaf) + ld(2, b"") + ld(2, url)
             + ld(3, ld(1, b"k") + ld(2, url + leaf))),
        Case("value-before-url", ld(1, leaf + url) + after, ANY_WIRE),
        Case("url-twice", ld(1, url + url + leaf) + after, ANY_WIRE),
        Case("unknown-field-3-after", ld(1, url + leaf + tag(3, 0) + vi(1)) + after,
             ANY_WIRE),
        Case("unknown-field-3-between", ld(1, url + tag(3, 0) + vi(1) + leaf),
             ANY_WIRE),
        Case("value-only", ld(1, leaf) + after),
        Case("unknown-type", ld(1, ld(1, b"t.Nope") + leaf) + after),
        Case("stranger-type", ld(1, ld(1, b"v.Stranger") + ld(2, tag(1, 0) + vi(1)))),
        Case("truncated-value", ld(1, url + tag(2, 2) + b"\x05\x08")),
        Case("corrupt-payload", ld(1, url + ld(2, b"\x08")) + after),
        Case("corrupt-payload-in-ra", ld(2, url + ld(2, b"\x08")) + ld(2, url + leaf)),
        Case("length-overruns-any", ld(1, url + tag(2, 2) + b"\x7f" + tag(1, 0)
                                      + vi(5)) + after),
        Case("url-length-overruns-any", ld(1, tag(1, 2) + b"\x7f" + b"t.Leaf")),
        Case("huge-length-in-payload",
             ld(1, url + ld(2, tag(2, 2) + vi(2**64 - 3))) + after),
        Case("huge-value-length", ld(1, url + tag(2, 2) + vi(2**64 - 5))),
        Case("url-bad-utf8", ld(1, ld(1, b"\xff/t.Leaf") + leaf)),
    ]


ACCEPT = _accept_cases()
REJECT = _reject_cases()
ORACLE_DECIDES = _oracle_decides_cases()
WIRES = _wire_cases()
HOST_CAP = 8     # at most one ACCEPT+WIRES case in eight may carry a HOST tag


# ---- comparison ---------------------------------------------------------------

_ANY = "google.protobuf.Any"
# Any payloads printed as {"@type":..., "value": X} by the oracle
_VALUE_PAYLOADS = (pc._DOUBLE_WKT | pc._STRING_WKT | {_ANY})


def _field_eq(a, b, fd, pool) -> bool:
    if fd.type == fd.TYPE_MESSAGE:
        return same_json(a, b, fd.message_type, pool)
    return pc._field_eq(a, b, fd)


def same_json(a, b, desc, pool) -> bool:
    """protojson_corpus.same_json, with an Any compared under the schema its
    "@type" names in ``pool``."""
    full = desc.full_name
    if full == _ANY:
        if not (isinstance(a, dict) and isinstance(b, dict)):
            return False
        if not a or not b:
            return a == b
        if "@type" not in a or a.get("@type") != b.get("@type"):
            return False
        try:
            pd = pool.FindMessageTypeByName(a["@type"].rsplit("/", 1)[-1])
        except KeyError:
            return False
        wrapper = (pd.file.name == "google/protobuf/wrappers.proto")
        if wrapper or pd.full_name in _VALUE_PAYLOADS:
            return (set(a) == set(b) == {"@type", "value"}
                    and same_json(a["value"], b["value"], pd, pool))
        return same_json({k: v for k, v in a.items() if k != "@type"},
                         {k: v for k, v in b.items() if k != "@type"}, pd, pool)
    if full.startswith("google.protobuf."):
        return pc.same_json(a, b, desc)
    if not (isinstance(a, dict) and isinstance(b, dict)) or a.keys() != b.keys():
        return False
    by_json = {fd.json_name: fd for fd in desc.fields}
    for k in a:
        fd = by_json.get(k)
        if fd is None:
            return False
        x, y = a[k], b[k]
        if fd.message_type is not None and fd.message_type.GetOptions().map_entry:
            vfd = fd.message_type.fields_by_name["value"]
            if not (isinstance(x, dict) and isinstance(y, dict)) or x.keys() != y.keys():
                return False
            if not all(_field_eq(x[m], y[m], vfd, pool) for m in x):
                return False
        elif fd.is_repeated:
            if not (isinstance(x, list) and isinstance(y, list)) or len(x) != len(y):
                return False
            if not all(_field_eq(p, q, fd, pool) for p, q in zip(x, y)):
                return False
        elif not _field_eq(x, y, fd, pool):
            return False
    return True


# ---- oracle + batch runners ---------------------------------------------------

def oracle_parse(env: Env, text: str):
    """json_format with the schema's pool -> message, or None if it raises
    (a WKT payload without "value" raises KeyError, not ParseError)."""
    try:
        return json_format.Parse(text, env.cls(), descriptor_pool=env.pool)
    except Exception:
        return None


def oracle_print(env: Env, wire: bytes) -> Optional[str]:
    try:
        msg = env.cls.FromString(wire)
        return json_format.MessageToJson(msg, indent=None, ensure_ascii=False,
                                         descriptor_pool=env.pool)
    except Exception:
        return None


def encode_verdicts(env: Env, cases: Sequence[Case], enc, pbs) -> dict:
    desc = env.cls.DESCRIPTOR
    out = {}
    for c, r, pb in zip(cases, enc, pbs):
        want = oracle_parse(env, c.data)

        def equal(pb=pb, want=want):
            try:
                got = env.cls.FromString(pb)
                g = json_format.MessageToDict(got, descriptor_pool=env.pool)
            except Exception as exc:
                return f"kernel wire does not parse/print: {exc!r} {pb!r}"
            o = json_format.MessageToDict(want, descriptor_pool=env.pool)
            if same_json(g, o, desc, env.pool):
                return None
            return f"\nkernel: {g}\noracle: {o}"

        out[c.id] = pc._verdict(c, int(r["status"]), want is not None, equal)
        if out[c.id]:
            out[c.id] += f"  [aux={int(r['aux'])}] input={c.data[:200]!r}"
    return out


def run_encode(env: Env, cases: Sequence[Case]) -> dict:
    """One k_json2pb batch over ``cases``; case id -> None | failure text."""
    enc, pbs = env.engine.encode_batch(
        [c.data.encode() for c in cases], mode=1,
        msg_indices=[env.idx] * len(cases), enforce=False)
    return encode_verdicts(env, cases, enc, pbs)


def envelope_bodies(env: Env, n: int) -> List[bytes]:
    return [json.dumps({"jsonrpc": "2.0", "id": i, "method": "tools/call",
                        "params": {"name": env.tool, "arguments": {}}}).encode()
            for i in range(n)]


def unwrap_envelope(o) -> str:
    resp = json.loads(o)
    assert resp["result"]["isError"] is False
    return resp["result"]["content"][0]["text"]


def decode_verdicts(env: Env, cases, wires, dec, outs, unwrap) -> dict:
    desc = env.cls.DESCRIPTOR
    out = {}
    for c, w, r, o in zip(cases, wires, dec, outs):
        want = oracle_print(env, w)

        def equal(o=o, want=want):
            try:
                text = unwrap(o)
                g = pc.loads(text)
            except Exception as exc:
                return f"kernel text is not JSON: {exc!r} {o!r}"
            if same_json(g, pc.loads(want), desc, env.pool):
                dups = pc.duplicate_members(text)
                return f"duplicate JSON members {dups}: {o!r}" if dups else None
            return f"\nkernel: {o!r}\noracle: {want!r}"

        out[c.id] = pc._verdict(c, int(r["status"]), want is not None, equal)
        if out[c.id]:
            out[c.id] += f"  wire={w.hex()[:200]}"
    return out


def run_decode(env: Env, cases: Sequence[Case], wires: Sequence[bytes],
               mode: int = 1) -> dict:
    """One k_pb2json batch; mode 0 first primes the request ids with an
    envelope encode batch and compares the text inside the envelope."""
    n = len(cases)
    if mode == 0:
        enc, _ = env.engine.encode_batch(envelope_bodies(env, n), mode=0)
        assert all(int(r["status"]) == 0 for r in enc)
        unwrap = unwrap_envelope
    else:
        unwrap = lambda o: o  # noqa: E731
    dec, outs = env.engine.decode_batch(list(wires), [env.idx] * n, mode=mode)
    res = decode_verdicts(env, cases, wires, dec, outs, unwrap)
    if mode == 0:
        for i, (c, o) in enumerate(zip(cases, outs)):
            if o is not None and res[c.id] is None and json.loads(o)["id"] != i:
                res[c.id] = f"envelope id {json.loads(o)['id']} in slot {i}"
    return res


def accept_wires(env: Env) -> List[bytes]:
    """The oracle's own serialisation of every ACCEPT payload."""
    return [json_format.Parse(c.data, env.cls(), descriptor_pool=env.pool)
            .SerializeToString() for c in ACCEPT]
