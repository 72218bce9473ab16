"""Case lists of test_wg_packed_chunks.py and test_gpu_packed_chunks.py: every size
from ``WG_DEC_PACK_CHUNK`` (``C``) and the 16 KB threshold, texts from ``repr`` / ``str``."""

import struct
from itertools import accumulate

import packed_runs_corpus as pr
import packed_varint_corpus as pv
import protojson_corpus as pc
from protojson_corpus import ld, tag, vi

from ggrmcp_amd.engine.hostsim import WG_DEC_MIN_BYTES, load_module

C, MAX_ITEMS = load_module().WG_DEC_PACK_CHUNK, load_module().WG_DEC_MAX_ITEMS
BIG, UNPOP, STRUCT = max(WG_DEC_MIN_BYTES, 2 * C), 4, 8
LONG = C * max(3, -(-BIG // C))  # a whole number of chunks: candidates at k * C

# kind -> (schema, field number, JSON name); c.Chunks has what p/v.Holder lack
OWN = ["fixed32", "sfixed32", "fixed64", "sfixed64", "int32", "uint32",
       "uint64", "sint32", "sint64", "bool"]
FIELD = {"double": ("p", 2, "top"), "float": ("p", 3, "f"),
         "int64": ("v", 2, "top"), "enum": ("v", 3, "e")}
FIELD.update({k: ("c", 3 + i, pc._camel(f"r_{k}")) for i, k in enumerate(OWN)})
KINDS = pr.FIXED_KINDS + pv.KINDS
WIDTH = {k: struct.calcsize(f) for k, f in pr.FMT.items()}


def make_holders(engine_factory) -> dict:
    """p.Holder, v.Holder and c.Chunks for ``packed_runs_corpus.run_holder``."""
    from google.protobuf import message_factory
    from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos
    from ggrmcp_amd.utils.protobuild import FileBuilder

    fb = FileBuilder("c/chunks.proto", "c")
    fb.message("Sub").field("x", 1, "int32").done()
    mb = fb.message("Chunks").map_field("m", 1, "string", "int32").field("lead", 2, "int32")
    for k in OWN:
        mb.field(f"r_{k}", FIELD[k][1], k, repeated=True)
    mb.field("sub", 13, "message", message="Sub").field("note", 14, "string").done()
    fb.service("ChunkService").method("Echo", "Chunks", "Chunks").done()
    pool = build_pool([fb.build()])
    infos = {m.tool_name(): m
             for m in extract_method_infos([fb.build()], pool, compat_names=False)}
    engine = engine_factory(infos)
    cls = message_factory.GetMessageClass(pool.FindMessageTypeByName("c.Chunks"))
    return {"p": pr.make_holder(engine_factory), "v": pv.make_holder(engine_factory),
            "c": (engine, cls, engine.tables.msg_index["c.Chunks"], next(iter(infos)))}


def take(kind: str, nbytes: int):
    """(encodings, texts) of elements of ``kind`` until ``nbytes`` are reached.  Doubles
    and floats are odd multiples of 1/16: ``repr`` is the protojson text."""
    n, fp = nbytes // WIDTH.get(kind, 1) + 1, kind in ("double", "float")
    vals = ([((i * 37) % 4001 - 2000) + (i % 8 * 2 + 1) / 16 for i in range(n)] if fp
            else pr.mixed_values(kind, n) if kind in WIDTH else pv.values(kind, n))
    txt = [repr(v) for v in vals] if fp else pv.texts(kind, vals).split(",")
    enc = [pr.body(kind, [v]) if kind in WIDTH else pv.body(kind, [v]) for v in vals]
    n = next(i for i, e in enumerate(accumulate(map(len, enc))) if e >= nbytes) + 1
    return enc[:n], txt[:n]


def run(kind: str, enc, txt):
    return ld(FIELD[kind][1], b"".join(enc)), '"%s":[%s]' % (FIELD[kind][2], ",".join(txt))


def _case(cid, kind, parts, items=None, mode=0, status=0, ends=None):
    """``items``: the probe's kinds, None = two packed chunks or more.  ``ends``: the
    wire is the run alone, and these are its elements' ends from the body's start."""
    return (cid, FIELD[kind][0], b"".join(p[0] for p in parts), mode, status,
            "{%s}" % ",".join(p[1] for p in parts), items, ends)


NOTE = (ld(14, b"n" * BIG), '"note":"%s"' % ("n" * BIG))  # routes a short run
LEAD, SUB = (tag(2, 0) + vi(7), '"lead":7'), (ld(13, tag(1, 0) + vi(5)), '"sub":{"x":5}')
_KEYS = ["k%05d" % i for i in range(3 * C // 12 + 1)]  # 12-byte entries: 3 chunks
MAP = (b"".join(ld(1, ld(1, k.encode()) + tag(2, 0) + vi(1)) for k in _KEYS),
       '"m":{%s}' % ",".join('"%s":1' % k for k in _KEYS))
_I32 = run("int32", *take("int32", BIG + 1))
_S64, _BOOL, _DBL = take("sint64", BIG), take("bool", BIG), take("double", BIG + 1)
# DM_UNPOPULATED prints what is absent from c.Chunks (sub has presence)
_FILL = [(b"", '"%s":[]' % FIELD[k][2]) for k in OWN]
_V, _1, _TEN, _MAX = FIELD["int64"][1], b"\x01", (2 * C + 64) // 10, '"%d"' % (2**64 - 1)

MIDDLE = _case("middle", "int32", [LEAD, _I32, NOTE])
SHORT = _case("short", "sfixed64", [run("sfixed64", *take("sfixed64", 2 * C - 8)), NOTE], [0, 0])
MAPPED = _case("map-run-message", "int32", [MAP, _I32, SUB])
CASES = (
    [_case(k, k, [run(k, *e)], ends=set(accumulate(map(len, e[0]))))
     for k in KINDS for e in [take(k, BIG + 1)]]
    # body lengths around k whole chunks, both widths; a ragged body
    + [_case(f"{kind}-{k}C{d:+d}w", kind,
             [run(kind, *take(kind, k * C + d * WIDTH[kind])), NOTE],
             [0, 0] if k * C + d * WIDTH[kind] < 2 * C else None)
       for kind in ("fixed64", "fixed32") for k in (2, 3) for d in (-1, 0, 1)]
    + [_case("ragged", "fixed64", [(ld(5, b"\x00" * (2 * C + 9)), ""), NOTE], status=pr.E_PARSE)]
    # the candidate on every byte of a ten-byte element, bodies of one length
    + [_case(f"sweep-{j}", "uint64",
             [run("uint64", [b"\x01"] * j + [vi(2**64 - 1)] * _TEN + [b"\x01"] * (16 - j),
                  ['"1"'] * j + [_MAX] * _TEN + ['"1"'] * (16 - j)), NOTE])
       for j in range(11)]
    + [_case("uint32-five-byte", "uint32",
             [run("uint32", [vi(2**32 - 5)] * -(-LONG // 5), [str(2**32 - 5)] * -(-LONG // 5))]),
       _case("nonminimal-zeros", "int32",
             [run("int32", [b"\x80\x00"] * (LONG // 2), ["0"] * (LONG // 2))]),
       _case("only", "int32", [_I32]), _case("first", "int32", [_I32, NOTE]),
       MIDDLE, _case("last", "int32", [LEAD, _I32]), MAPPED,
       _case("two-records", "sint64",
             [(run("sint64", *_S64)[0] * 2, run("sint64", _S64[0], _S64[1] * 2)[1])], [0]),
       _case("packed-then-unpacked", "bool",
             [(run("bool", *_BOOL)[0] + tag(12, 0) + vi(1),
               run("bool", _BOOL[0], _BOOL[1] + ["true"])[1])], [0]),
       SHORT,
       _case("nested", "double", [(ld(1, ld(1, b"".join(_DBL[0]))),
                                   '"run":{"d":[%s]}' % ",".join(_DBL[1]))], [0])]
    # malformed varints; twenty continuation bytes stop the split
    + [_case(cid, "int64", [(ld(_V, body), "")], items, status=pr.E_PARSE)
       for cid, body, items in [
           ("eleven-bytes", _1 * (C - 5) + b"\xff" * 10 + _1 * (LONG - C - 5), None),
           ("eleven-bytes-later", _1 * (2 * C - 5) + b"\xff" * 10 + _1 * (LONG - 2 * C - 5), None),
           ("split-stops", _1 * (2 * C - 5) + b"\x80" * 20 + _1 * (LONG - 2 * C - 15), [2, 2]),
           ("no-terminator", _1 * (LONG - 1) + b"\x80", None),
           ("continuation-tail", _1 * (LONG - 20) + b"\x80" * 20, None)]]
    + [_case(f"middle-flags-{mode}", "int32",
             [(b"", '"m":{}'), LEAD] + _FILL[:4] + [_I32] + _FILL[5:] + [NOTE], mode=mode)
       for mode in (UNPOP, UNPOP | STRUCT)]
)
# CPU build only: more chunks than items; a candidate in the last ten bytes
_CAP = run("bool", [b"\x01" * ((MAX_ITEMS + 8) * C)], ["true"] * ((MAX_ITEMS + 8) * C))
_K = C // 8  # chunks of C + 8 bytes: the last candidate lies 5 bytes from the end
_END = _K * (C + 8) + 5
CPU_ONLY = [
    _case("item-cap", "bool", [(b"", '"m":{}'), (b"", '"lead":0')] + _FILL[:9]
          + [_CAP, (b"", '"note":""')], mode=UNPOP, ends=range((MAX_ITEMS + 8) * C + 1)),
    _case("candidate-at-the-end", "int64",
          [run("int64", [b"\x01" * (_END - 6), b"\x80" * 5 + b"\x01"],
               ['"1"'] * (_END - 6) + ['"%d"' % (1 << 35)])], [2] * _K),
]
# (wire, (status, pad)): an empty packed run takes the in-block classic pass
BATCH = [(MIDDLE[2], (0, 1)), (SHORT[2], (0, 1)), (ld(FIELD["int32"][1], b"") + NOTE[0], (0, 2)),
         (LEAD[0], (0, 0)), (MAPPED[2], (0, 1))]
