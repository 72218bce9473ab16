"""Values, wires and expected texts (``str()`` / ``'"%d"'`` / ``true|false`` /
the ``Color`` names) for the packed varint run tests, CPU build and gfx950."""

import protojson_corpus as pc
from protojson_corpus import ld, tag, vi

KINDS = ["int32", "int64", "uint32", "uint64", "sint32", "sint64", "bool", "enum"]
RUN_LENGTHS = [1, 2, 63, 64, 65, 128, 129, 200]
COLOR = {0: "C_ZERO", 1: "C_ONE", -1: "C_NEG"}

# encodings of 1, 2, 5 and 10 bytes where the kind has them, range edges,
# both zigzag extremes; bool as the raw varint; enum known, unknown, negative.
# Every length is coprime to 7 (values() below)
POOL = {
    "int32": [0, 1, -1, 127, 128, 300, 2**31 - 1, -2**31, 16384, 2**28, -5],
    "int64": [0, 1, -1, 300, 2**63 - 1, -2**63, 2**34, 2**28, 127, 128, -77],
    "uint32": [0, 1, 127, 128, 300, 2**32 - 1, 2**28, 16383, 99],
    "uint64": [0, 1, 128, 2**64 - 1, 2**63, 2**35, 300, 2**28, 9],
    "sint32": [0, -1, 1, -64, 64, 2**31 - 1, -2**31, 300, -2**27],
    "sint64": [0, -1, 1, 2**63 - 1, -2**63, -300, 2**33, 63, -2**27],
    "bool": [0, 1, 2, 1 << 40, 2**64 - 1],
    "enum": [0, 1, -1, 7, -9, 2**31 - 1],
}


def values(kind: str, n: int) -> list:
    pool = POOL[kind]
    return [pool[(i * 7 + 3) % len(pool)] for i in range(n)]


def body(kind: str, vals) -> bytes:
    zz = kind in ("sint32", "sint64")
    return b"".join(vi(pc._zz(v) if zz else v) for v in vals)


def packed(kind: str, vals) -> bytes:
    return ld(pc.F[f"r_{kind}"], body(kind, vals))


def texts(kind: str, vals) -> str:
    if kind == "bool":
        return ",".join("true" if v else "false" for v in vals)
    if kind == "enum":
        return ",".join('"%s"' % COLOR[v] if v in COLOR else str(v) for v in vals)
    return ",".join(('"%d"' if kind.endswith("64") else "%d") % v for v in vals)


def expected(kind: str, vals) -> bytes:
    """The bare (mode 1) decode of ``packed(kind, vals)``."""
    return ('{"%s":[%s]}' % (pc._camel(f"r_{kind}"), texts(kind, vals))).encode()


def device_cases():
    runs = [(k, values(k, n)) for k in KINDS for n in RUN_LENGTHS]
    return [packed(k, v) for k, v in runs], [expected(k, v) for k, v in runs]


ALL_ONES = b"\xff" * 9 + b"\x7f"  # ten bytes, 2^64 - 1 after the dropped bits
_MIX = {c.id: c.data for c in pc.WIRES}
# (wire, bare text): non-minimal encodings, 300 ten-byte and 300 one-byte
# elements, then the protojson corpus' packed / unpacked / packed mix of one
# field and its empty run before a full one, which keep their commas
EXACT = [
    (ld(pc.F["r_uint64"], b"\x80\x00" + ALL_ONES + b"\x81\x80\x80\x00"),
     expected("uint64", [0, 2**64 - 1, 1])),
    (ld(pc.F["r_int32"], b"\x80\x00" + ALL_ONES), expected("int32", [0, -1])),
    (packed("int64", [-3] * 300), expected("int64", [-3] * 300)),
    (packed("uint32", [7] * 300), expected("uint32", [7] * 300)),
    (_MIX["packed-mixed-runs"], b'{"rInt32":[1,2,3,4]}'),
    (_MIX["packed-empty-then-data"], b'{"rInt32":[9]}'),
]
FILL = [("uint32", 7, 200), ("int64", -3, 100)]

_GOOD = [vi(v) for v in values("int64", 50)]
_R = pc.F["r_int64"]
# each is E_PARSE on the serial path: an 11-byte varint as the first, the 40th
# and the last element; a tail of 1..9 continuation bytes; a run that ends
# inside an element which the next field's tag would terminate for a reader
# that looked past the run's end
MALFORMED = (
    [ld(_R, b"".join(_GOOD[:at]) + b"\xff" * 10 + b"\x01" + b"".join(_GOOD[at + 1:]))
     for at in (0, 39, 49)]
    + [ld(_R, b"".join(_GOOD[:3]) + b"\x80" * n) for n in range(1, 10)]
    + [ld(_R, vi(5) + b"\x80") + tag(pc.F["opt_i32"], 0) + vi(1)])

# 65 elements: 64 one-digit texts in quotes, then the longest int64 text
OVERFLOW_RUN = [i % 10 for i in range(64)] + [-2**63]


def make_holder(engine_factory):
    """v.Holder for ``packed_runs_corpus.run_holder``: a nested run, two on top."""
    from google.protobuf import message_factory

    from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos
    from ggrmcp_amd.utils.protobuild import FileBuilder

    fb = FileBuilder("v/holder.proto", "v")
    fb.enum("Color", [("C_ZERO", 0), ("C_ONE", 1), ("C_NEG", -1)])
    (fb.message("Run").field("a", 1, "int32", repeated=True)
       .field("z", 2, "sint64", repeated=True).done())
    (fb.message("Holder").field("run", 1, "message", message="Run")
       .field("top", 2, "int64", repeated=True)
       .field("e", 3, "enum", enum="Color", repeated=True).done())
    fb.service("HolderService").method("Echo", "Holder", "Holder").done()
    fdps = [fb.build()]
    pool = build_pool(fdps)
    infos = {m.tool_name(): m
             for m in extract_method_infos(fdps, pool, compat_names=False)}
    cls = message_factory.GetMessageClass(pool.FindMessageTypeByName("v.Holder"))
    engine = engine_factory(infos)
    return engine, cls, engine.tables.msg_index["v.Holder"], next(iter(infos))


def holder_wires(cls) -> dict:
    """Two responses past 16 KB and a small one with descending fields."""
    a, z = values("int32", 3000), values("sint64", 1500)
    top, e = values("int64", 4000), values("enum", 700)
    return {
        "nested": cls(run={"a": a, "z": z}).SerializeToString(),
        "top": cls(top=top, e=e).SerializeToString(),
        "descending": (cls(e=e[:70]).SerializeToString()
                       + cls(top=top[:70]).SerializeToString()
                       + cls(run={"a": a[:70], "z": z[:70]}).SerializeToString()),
    }
