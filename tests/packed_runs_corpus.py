"""Values and wire helpers for the packed fixed-width run tests
(``test_packed_fixed_runs.py`` on the CPU build,
``test_gpu_packed_fixed_runs.py`` on gfx950).  Plain data: seeded
``random.Random`` and ``struct`` only.
"""

import random
import struct
from decimal import ROUND_FLOOR, Decimal
from typing import List

import protojson_corpus as pc
from protojson_corpus import ld

E_PARSE, E_OVERFLOW = pc.E_PARSE, pc.E_OVERFLOW
FIXED_KINDS = ["double", "float", "fixed32", "sfixed32", "fixed64", "sfixed64"]
FMT = {"double": "<d", "float": "<f", "fixed32": "<I", "sfixed32": "<i",
       "fixed64": "<Q", "sfixed64": "<q"}


def _d(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _f(bits: int) -> float:
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _every_exponent(n_exp: int, mant_bits: int, sign_bit: int, conv,
                    seed: int) -> List[float]:
    """Mantissa fields 0, 1, all-ones and one seeded random value at every
    finite biased exponent, in both signs; zero itself left out."""
    rng = random.Random(seed)
    ones = (1 << mant_bits) - 1
    out = []
    for e in range(n_exp):
        for m in (0, 1, ones, rng.randrange(2, ones)):
            if e == 0 and m == 0:
                continue
            bits = e << mant_bits | m
            out += [conv(bits), conv(bits | 1 << sign_bit)]
    return out


# test 1: every binary exponent, subnormals (biased exponent 0) included, and
# the first 64 subnormals: there the candidate has one or two digits and a
# multiple of ten beside it can be the shortest (10 * 2^-1074 = 5e-323)
DOUBLES = _every_exponent(2047, 52, 63, _d, 11) + [_d(b) for b in range(1, 65)]
FLOATS = _every_exponent(255, 23, 31, _f, 12) + [_f(b) for b in range(1, 65)]


def random_doubles(n: int, seed: int) -> List[float]:
    """Random bit patterns with a non-zero mantissa field inside the range
    the singular emitter prints on the device."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        bits = rng.getrandbits(64)
        v = _d(bits)
        if bits & (1 << 52) - 1 and 1e-306 <= abs(v) <= 1e308:
            out.append(v)
    return out


# one value per decimal exponent -8..22 in both signs: every text layout
LAYOUT_SWEEP = [s * float(f"1.2345e{e}") for e in range(-8, 23) for s in (1, -1)]

INT_EDGES = {
    "fixed32": [0, 1, 2**32 - 1],
    "sfixed32": [0, 1, 2**31 - 1, -2**31, -1],
    "fixed64": [0, 1, 2**64 - 1],
    "sfixed64": [0, 1, 2**63 - 1, -2**63, -1],
}
NONFINITE = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0]

RUN_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 200]


def mixed_values(kind: str, n: int) -> list:
    """``n`` values of ``kind`` whose texts run from 1 to 24 bytes, in an
    order that carries unequal lengths across every window edge."""
    if kind == "double":
        pool = [0.0, 5.0, -0.0, 1e22, -1.5] + DOUBLES[::37] + NONFINITE
    elif kind == "float":
        pool = [0.0, 5.0, -0.0, 1e22, -1.5] + FLOATS[::7] + NONFINITE
    else:
        lo, hi = pc.INT_RANGES[kind]
        pool = INT_EDGES[kind] + [hi // 10**k for k in range(1, 19, 2)] \
            + [lo // 10**k for k in range(1, 19, 2)]
    return [pool[(i * 7 + 3) % len(pool)] for i in range(n)]


def body(kind: str, values) -> bytes:
    return b"".join(struct.pack(FMT[kind], v) for v in values)


def packed(kind: str, values) -> bytes:
    """One packed run of ``t.Sink.r_<kind>``."""
    return ld(pc.F[f"r_{kind}"], body(kind, values))


def unpacked(kind: str, values) -> bytes:
    wt = 1 if FMT[kind][1] in "dQq" else 5
    return b"".join(pc.tag(pc.F[f"r_{kind}"], wt) + struct.pack(FMT[kind], v)
                    for v in values)


# run bodies that are no multiple of the element width: 8k+1..8k+7, 4k+1..4k+3
BAD_BODIES = [(kind, w * k + r)
              for kind, w in (("double", 8), ("sfixed64", 8), ("float", 4),
                              ("fixed32", 4))
              for k in (0, 3, 64) for r in range(1, w)]

# 65 elements: 64 short texts, then the longest double text there is
OVERFLOW_RUN = [float(i % 10) for i in range(64)] + [-1.2345678901234567e-6]


def decode_slot(env, wire: bytes, scratch_bytes: int, mode: int = 1):
    """One t.Sink slot through the engine's raw decode entry with a scratch
    region of exactly ``scratch_bytes``: (status, output or None)."""
    import numpy as np

    from ggrmcp_amd.engine.batch import DECODE_DTYPE

    off = lambda n: np.asarray([0, n], dtype=np.uint32)  # noqa: E731
    raw, fin = env.engine._eng.decode(
        wire, off(len(wire)), off(scratch_bytes), off(16 * len(wire) + 2048),
        np.asarray([env.sink_idx], dtype=np.int32), np.zeros(1, dtype=np.int32),
        mode)
    r = np.frombuffer(raw.tobytes(), dtype=DECODE_DTYPE)[0]
    if int(r["status"]):
        return int(r["status"]), None
    return 0, bytes(memoryview(fin)[r["out_off"]:r["out_off"] + r["out_len"]])


DM_UNPOPULATED, DM_REORDER = 4, 16


def device_wires() -> List[bytes]:
    """Every kind at every run length, mixed text lengths."""
    return [packed(k, mixed_values(k, n)) for k in FIXED_KINDS for n in RUN_LENGTHS]


def run_batch(env, wires, mode: int, filler=None):
    """One decode batch -> [(status, pad, output)].  With ``filler`` (a byte
    count) a filler slot of that many more bytes leads the batch, so every
    slot start shifts with it; its own result is left out.  An envelope batch
    first primes the request ids with an encode batch."""
    lead = [] if filler is None else [ld(pc.F["opt_str"], b"f" * filler)]
    wires = lead + list(wires)
    if mode & 3 == 0:
        bodies = [b'{"jsonrpc":"2.0","id":%d,"method":"tools/call","params":'
                  b'{"name":"%s","arguments":{}}}' % (i, env.sink_tool.encode())
                  for i in range(len(wires))]
        enc, _ = env.engine.encode_batch(bodies, mode=0)
        assert all(int(r["status"]) == 0 for r in enc)
    dec, outs = env.engine.decode_batch(wires, [env.sink_idx] * len(wires), mode=mode)
    return [(int(r["status"]), int(r["pad"]), o)
            for r, o in zip(dec, outs)][len(lead):]


def holder_fdp():
    """p.Holder: a packed run inside a nested message and two at the top."""
    from ggrmcp_amd.utils.protobuild import FileBuilder

    fb = FileBuilder("p/holder.proto", "p")
    (fb.message("Run").field("d", 1, "double", repeated=True)
       .field("q", 2, "sfixed64", repeated=True).done())
    (fb.message("Holder").field("run", 1, "message", message="Run")
       .field("top", 2, "double", repeated=True)
       .field("f", 3, "float", repeated=True).done())
    fb.service("HolderService").method("Echo", "Holder", "Holder").done()
    return fb.build()


def make_holder(engine_factory):
    """(engine, p.Holder class, its table index, its tool name)."""
    from google.protobuf import message_factory

    from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos

    fdps = [holder_fdp()]
    pool = build_pool(fdps)
    infos = {m.tool_name(): m
             for m in extract_method_infos(fdps, pool, compat_names=False)}
    engine = engine_factory(infos)
    cls = message_factory.GetMessageClass(pool.FindMessageTypeByName("p.Holder"))
    return engine, cls, engine.tables.msg_index["p.Holder"], next(iter(infos))


def holder_wires(cls) -> dict:
    """Responses past the workgroup kernel's 16 KB threshold, and one small
    wire whose fields arrive in descending order."""
    d, q = mixed_values("double", 1500), mixed_values("sfixed64", 700)
    top, f = mixed_values("double", 2100), mixed_values("float", 300)
    return {
        "nested": cls(run={"d": d, "q": q}).SerializeToString(),
        "top": cls(top=top, f=f).SerializeToString(),
        "descending": (cls(f=f[:70]).SerializeToString()
                       + cls(top=top[:70]).SerializeToString()
                       + cls(run={"d": d[:70], "q": q[:70]}).SerializeToString()),
    }


def run_holder(holder, wire: bytes, mode: int):
    """One p.Holder envelope slot -> (status, pad, output)."""
    engine, _, idx, tool = holder
    body = (b'{"jsonrpc":"2.0","id":1,"method":"tools/call","params":'
            b'{"name":"%s","arguments":{}}}' % tool.encode())
    enc, _ = engine.encode_batch([body], mode=0)
    assert int(enc[0]["status"]) == 0
    dec, outs = engine.decode_batch([wire], [idx], mode=mode)
    return int(dec[0]["status"]), int(dec[0]["pad"]), outs[0]


def elements(text: str, kind: str) -> List[str]:
    """The element texts of ``{"rKind":[...]}`` (quotes kept)."""
    head = '{"%s":[' % pc._camel(f"r_{kind}")
    assert text.startswith(head) and text.endswith("]}"), text[:80]
    return text[len(head):-2].split(",")


def sig_digits(text: str) -> str:
    """Significant digits of a JSON number, zeros stripped at both ends."""
    m = text.lstrip("-").lower().split("e")[0].replace(".", "")
    return m.strip("0")


def shortest_float32(v: float) -> str:
    """The decimal of fewest significant digits that parses back to the
    float32 ``v``; of two with that many digits the closer to ``v``.  Both
    neighbours of ``v`` on the p-digit grid are tried: below a power of two
    the rounding interval is lopsided and only the farther one may fit."""
    want = struct.pack("<f", abs(v))
    d = Decimal(abs(v))
    for p in range(1, 10):
        step = Decimal(1).scaleb(d.adjusted() - p + 1)
        lo = d.quantize(step, rounding=ROUND_FLOOR)
        fits = [c for c in (lo, lo + step)
                if c < _FLT_TOP and struct.pack("<f", float(c)) == want]
        if fits:  # a tie goes to the even digit
            return str(min(fits, key=lambda c: (abs(c - d), c / step % 2)))
    raise AssertionError(v)


# FLT_MAX plus half a unit: from here on struct.pack raises
_FLT_TOP = Decimal("3.4028235677973366e38")
