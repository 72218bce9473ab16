"""Texts and the Python reference for packed arrays in the workgroup encode
kernel (``test_wg_packed_encode_host.py`` on the CPU build,
``test_gpu_wg_packed_encode.py`` on gfx950).  Plain data over t.Sink; the
reference wire is ``struct.pack`` / a varint of ``float(text)`` /
``int(text)`` behind the tag and the kernel's 3-byte length.
"""

from typing import List, Sequence

import packed_encode_corpus as pe
import protojson_corpus as pc

KINDS = ["double", "float", "int32", "sint64", "uint64", "fixed32", "bool", "enum"]
NUMERIC = KINDS[:6]                      # the kinds that take quoted numbers
_COLOR = {"C_ZERO": 0, "C_ONE": 1, "C_NEG": -1}

ELEMENT = {
    "double": lambda i: repr(i * 0.37 + 0.001),
    "float": lambda i: repr(i * 0.25 + 0.125),
    "int32": lambda i: str(i % 10),              # one-byte varints, "1," text
    "sint64": lambda i: str(-(i * 7919) - 1),
    "uint64": lambda i: str(2 ** 40 + i),
    "fixed32": lambda i: str(i * 65537 % 2 ** 32),
    "bool": lambda i: "true" if i % 3 else "false",
    "enum": lambda i: ['"C_ONE"', "1", '"C_NEG"', "0", "-1"][i % 5],
}


def elements(kind: str, nbytes: int) -> List[str]:
    """Element texts of ``kind`` whose array text is about ``nbytes`` long."""
    out, size = [], 0
    while size < nbytes:
        out.append(ELEMENT[kind](len(out)))
        size += len(out[-1]) + 1
    return out


def field_name(kind: str) -> str:
    return pc._camel(f"r_{kind}")


def field_index(kind: str) -> int:
    """Index of r_<kind> in t.Sink's field table (numbers run from 1)."""
    return pc.F[f"r_{kind}"] - 1


def record(kind: str, texts: Sequence[str]) -> bytes:
    """Tag, 3-byte length and payload of one array of element texts."""
    if kind not in ("bool", "enum"):
        return pe.ref_wire(kind, texts)
    out = b""
    for t in texts:
        t = t.strip().strip('"')
        v = {"true": 1, "false": 0}[t] if kind == "bool" else \
            _COLOR[t] if t in _COLOR else int(t)
        out += pc.vi(v % 2 ** 64)
    n = len(out)
    slot = bytes([n & 0x7F | 0x80, n >> 7 & 0x7F | 0x80, n >> 14 & 0x7F])
    return pc.tag(pc.F[f"r_{kind}"], 2) + slot + out


# ---- the device tier: arguments of 9 to 10 KB, the smallest that reach the
# multi-wave scanner; more than 513 elements and at least two chunks ----------

GPU_BYTES = 9300
# 24-byte keys: an entry's wire (34 bytes) stays under 5/4 of its text (31),
# the room an item and a slot get
BIG_MAP = "{%s}" % ",".join('"key%021d":%d' % (i, i) for i in range(600))
BIG_MSGS = "[%s]" % ",".join('"%d.000000001s"' % (100 + i) for i in range(600))
assert len(BIG_MAP) >= 8192 + 256 and len(BIG_MSGS) >= 8192 + 256
CAP_LIFT_DOCS = ['{"mString":%s}' % BIG_MAP, '{"rDur":%s}' % BIG_MSGS]


def quoted_some(kind: str, texts: Sequence[str]) -> List[str]:
    out = [f'"{t}"' if i % 5 == 2 else t for i, t in enumerate(texts)]
    if kind in pe.FP_KINDS:
        out[7::50] = ['"NaN"'] * len(out[7::50])
    return out


def accept_docs(kind: str):
    """[(shape, arguments text, element texts)] for one kind."""
    el = elements(kind, GPU_BYTES)
    assert len(el) > 513 and len(",".join(el)) >= 2 * 4096 + 256, kind
    name = field_name(kind)
    docs = [
        ("alone", '{"%s":[%s]}' % (name, ",".join(el)), el),
        ("between", '{"optI32":7,"%s":[%s],"optStr":"x"}' % (name, ",".join(el)), el),
        ("beside-map", '{"mString":%s,"%s":[%s]}' % (BIG_MAP, name, ",".join(el)), el),
        ("whitespace", '{"%s" : [ %s\t]\n}' % (name, " ,\n".join(el)), el),
    ]
    if kind in NUMERIC:
        q = quoted_some(kind, el)
        docs.append(("quoted", '{"%s":[%s]}' % (name, ",".join(q)), q))
    return docs


def _ones(n: int) -> List[str]:
    return ["1"] * n


def _with(texts: List[str], at: int, odd: str) -> str:
    return ",".join(texts[:at] + [odd] + texts[at + 1:])


# the offending element sits past the first 4096-byte mark, so in chunk two
_AT = 3000
# (id, arguments text, the oracle refuses it too)
REFUSALS = [
    ("float-1e999", '{"rFloat":[%s]}' % _with(_ones(4700), _AT, "1e999"), True),
    ("string-x", '{"rInt32":[%s]}' % _with(_ones(4700), _AT, '"x"'), True),
    ("two-commas", '{"rInt32":[%s]}' % _with(_ones(4700), _AT, "1,"), True),
    ("trailing-comma", '{"rInt32":[%s,]}' % ",".join(_ones(4700)), True),
    ("nested", '{"rInt32":[%s]}' % _with(_ones(4700), _AT, "[2]"), True),
    # the array never gets its ']': a '}' stands there.  (With nothing there
    # the envelope itself is unbalanced, phase A answers E_PARSE before any
    # scan and the slot carries SR_WG_ITEMS, as every envelope error does.)
    ("no-closer", '{"rInt32":[%s}}' % ",".join(_ones(4700)), True),
    # eight bytes of wire for two of text: past the item's and the slot's room
    ("overflow", '{"rDouble":[%s]}' % ",".join(["0"] * 4700), False),
]
assert all(len(d) >= 8192 + 1024 for _, d, _ in REFUSALS)

# ---- the CPU tier: ~200 elements, cut at 0, 1, 2 and 7 commas ----------------

HOST_ELEMENTS = 200
CUT_COUNTS = [0, 1, 2, 7]


def comma_cuts(text: str, n: int) -> List[int]:
    """``n`` comma offsets of ``text`` (no strings with commas in it), spread
    evenly."""
    commas = [i for i, ch in enumerate(text) if ch == ","]
    return [commas[(k + 1) * len(commas) // (n + 1)] for k in range(n)]
