"""Texts and the Python reference for the packed-array encode tests
(``test_packed_encode_runs.py`` on the CPU build,
``test_gpu_packed_encode_runs.py`` on gfx950).  Plain data: lists, seeded
``random.Random``, ``struct``, ``float()`` and ``int()``.
"""

import random
import struct
from typing import List, Sequence

import protojson_corpus as pc

E_PARSE, E_INVALID, E_UNSUPPORTED, E_OVERFLOW = 1, 4, 6, 7
FP_KINDS = ["double", "float"]
INT_KINDS = list(pc.INT_RANGES)
KINDS = FP_KINDS + INT_KINDS


def doc(kind: str, texts: Sequence[str], sep: str = ",") -> str:
    return '{"%s":[%s]}' % (pc._camel(f"r_{kind}"), sep.join(texts))


def quoted(texts: Sequence[str]) -> List[str]:
    return [t if t.startswith('"') else f'"{t}"' for t in texts]


def ref_wire(kind: str, texts: Sequence[str]) -> bytes:
    """The kernel's wire for one array: tag, 3-byte length slot, payload from
    ``float(text)`` / ``int(text)``."""
    out = b""
    for t in texts:
        t = t.strip().strip('"')
        if kind in FP_KINDS:
            out += struct.pack("<d" if kind == "double" else "<f", float(t))
            continue
        v = int(t) if t.lstrip("-").isdigit() else int(float(t))
        if kind.startswith("sint"):
            v = pc._zz(v)
        if "fixed" in kind:
            width = 8 if kind.endswith("64") else 4
            out += (v % 256 ** width).to_bytes(width, "little")
        else:
            out += pc.vi(v % 2 ** 64)
    n = len(out)
    slot = bytes([n & 0x7F | 0x80, n >> 7 & 0x7F | 0x80, n >> 14 & 0x7F])
    return pc.tag(pc.F[f"r_{kind}"], 2) + slot + out


def encode(env, docs: Sequence[str], filler=None):
    """One ``encode_batch(mode=1)`` over t.Sink texts -> [(status, err_pos,
    aux, wire)]; ``filler`` bytes of a leading slot shift every slot start."""
    lead = [] if filler is None else ['{"optStr":"%s"}' % ("f" * filler)]
    enc, pbs = env.engine.encode_batch(
        [d.encode() for d in lead + list(docs)], mode=1,
        msg_indices=[env.sink_idx] * (len(lead) + len(docs)), enforce=False)
    return [(int(r["status"]), int(r["err_pos"]), int(r["aux"]), pb)
            for r, pb in zip(enc, pbs)][len(lead):]


def check_exact(env, kind, arrays, filler=None):
    """Every array of element texts: status 0 and the reference's bytes."""
    got = encode(env, [doc(kind, a) for a in arrays], filler)
    for a, (status, _, _, wire) in zip(arrays, got):
        assert status == 0, (status, a[:4])
        assert wire == ref_wire(kind, a), a[:4]


# ---- test 1: the three host-escape rules, now on the device -------------------

HOST_RULE_CASES = ["dbl-denormal", "dbl-max", "dbl-long-mantissa"]
LONG_TEXTS = ["1.7976931348623157081452742373170435e308",
              "2.22507385850720138309023271733240406e-308",
              "0.1000000000000000055511151231257827"]
_EXT = ["5e-324", "2.2250738585072014e-308", "1.7976931348623157e308",
        "-1.7976931348623157e308"] + LONG_TEXTS
EXTREMES_65 = [_EXT[i % len(_EXT)] for i in range(65)]
TIE_DOC = doc("double", ["9007199254740993.0000000000000000001"])

# ---- test 2: every binary exponent, three spellings ---------------------------


def _spellings(n_exp: int, mant_bits: int, fmt: str, seed: int) -> List[str]:
    rng = random.Random(seed)
    out = []
    for e in range(n_exp):
        bits = e << mant_bits | rng.getrandbits(mant_bits) | (e == 0)
        v = struct.unpack(fmt, bits.to_bytes(struct.calcsize(fmt), "little"))[0]
        if rng.random() < 0.5:
            v = -v
        out += [repr(v), "%.17e" % v, "%.18e" % v]  # %.18e: 19 digits
    return out


DOUBLE_TEXTS = _spellings(2047, 52, "<d", 21)
FLOAT_TEXTS = _spellings(255, 23, "<f", 22)

# ---- test 3: window geometry --------------------------------------------------

COUNTS = [1, 63, 64, 65, 129]
WS_RUNS = [0, 1, 63, 300]


def pool(kind: str) -> List[str]:
    """Element texts of 1 to 25 bytes: at 25 bytes ten fill a 256-byte
    stretch and the eleventh straddles its edge.  Integer kinds: the extremes
    as numbers and as strings, and varints of every length from 1 to 10."""
    if kind in FP_KINDS:
        out = ["0", "-0.0", "1.5", '"NaN"', '"-Infinity"', '"Infinity"', "1e-7",
               '"2.5e3"', "-1.2345678901234567e-200", "3.4028234663852886e38",
               "0.000001234567890123456", "-7.00649232162408535e-46",
               "16777217", "1E+2", "-0e0", "123456789012345678901234"]
        return out
    lo, hi = pc.INT_RANGES[kind]
    vals = [lo, hi, 0, 1] + [hi >> s for s in range(3, 64, 7) if hi >> s] \
        + [lo >> s for s in range(1, 64, 9) if lo]
    return [str(v) if i % 3 else f'"{v}"' for i, v in enumerate(vals)] + ["-0"]


def geometry_docs(kind: str) -> List[str]:
    p = pool(kind)
    docs = [doc(kind, [p[(i * 5 + n) % len(p)] for i in range(n)]) for n in COUNTS]
    for ws in WS_RUNS[1:]:
        # a long run after every 16th separator, a short one before the others
        el = [p[i % len(p)] for i in range(65)]
        body = "".join(t + (" " * ws + "," + "\n" * ws if i % 16 == 0 else "\t,")
                       for i, t in enumerate(el[:-1])) + el[-1] + " " * ws
        docs.append('{"%s":[%s%s]}' % (pc._camel(f"r_{kind}"), "\r" * ws, body))
    return docs


def doc_texts(d: str) -> List[str]:
    return d[d.index("[") + 1:d.rindex("]")].split(",")


# ---- test 4: declined pieces --------------------------------------------------

ODD_AT = [0, 63, 64]
ODD_OK = ["1.0", "1e2"]                       # int32 array: status 0
# int32 array; the status the serial element gives for the odd one
ODD_BAD = [("2147483648", E_INVALID), ('"1,2"', E_INVALID),
           ('"\\u0031"', E_UNSUPPORTED), ("", E_PARSE), ("tru", E_PARSE)]


def odd_doc(odd: str, at: int, close: str = "]}") -> str:
    el = [str(i) for i in range(66)]
    el[at] = odd
    return '{"rInt32":[%s%s' % (",".join(el), close)


OVERFLOW_DOC = doc("double", ["0"] * 65)

# ---- test 5: one request over the workgroup threshold -------------------------

WG_TEXTS = (EXTREMES_65 + [repr(i / 7) for i in range(64)])
WG_DOC = ('{"rDouble":[%s],"rBytes":[%s]}'
          % (",".join(WG_TEXTS), ",".join(['"%s"' % ("QUJD" * 25)] * 170)))
assert len(WG_TEXTS) == 129 and len(WG_DOC) >= 16384 + 2048
