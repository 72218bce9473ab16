"""Double exactness fuzz (hostsim, CPU): the kernels must FORMAT doubles
as the shortest decimal that parses back to the same double, and PARSE
JSON decimals correctly rounded — across random bit patterns, ratios,
long mantissas, and extreme exponents.  These suites found and pinned
three real bugs in round 2 (17-digit blocks off by one, >2^53 mantissa
double-rounding, a DBL_MAX NaN collapse); keep them green."""

import json
import math
import random
import struct

import pytest

from google.protobuf import descriptor_pb2

from ggrmcp_amd.backend.discovery import ServiceDiscoverer
from ggrmcp_amd.config import Config
from ggrmcp_amd.engine.cpu_ref import CpuTranscoder
from ggrmcp_amd.engine.hostsim import HostSimEngine
from ggrmcp_amd.utils.synthetic import synthetic_fdp


@pytest.fixture(scope="module")
def env():
    cfg = Config.default()
    d = ServiceDiscoverer(cfg)
    fds = descriptor_pb2.FileDescriptorSet()
    fds.file.extend([synthetic_fdp()])
    d.load_descriptor_blob(fds.SerializeToString())
    eng = HostSimEngine(d.tools)
    cpu = CpuTranscoder()
    mi = d.tools["bench_echoservice_echo"]
    desc = mi.input_descriptor.fields_by_name["nested"].message_type
    idx = eng.tables.msg_index["bench.Inner"]
    return eng, cpu, desc, idx


def _gen_double(rng):
    k = rng.random()
    if k < 0.25:
        while True:
            v = struct.unpack(">d", struct.pack(">Q", rng.getrandbits(64)))[0]
            if math.isfinite(v) and abs(v) <= 1e308 and (
                    v == 0 or abs(v) >= 1e-306):
                return v
    if k < 0.5:
        return (rng.randint(1, 10**6) / rng.randint(1, 10**6)
                * 10 ** rng.randint(-12, 12))
    if k < 0.75:
        return round(rng.uniform(-1e6, 1e6), rng.randint(0, 12))
    return rng.random() * 10 ** rng.randint(-300, 300)


def test_format_shortest_roundtrip(env):
    """decode: kernel text must parse back to the exact double AND use no
    more significant digits than Python's shortest repr."""
    eng, cpu, desc, idx = env
    rng = random.Random(2024)
    vals = [_gen_double(rng) for _ in range(20000)]
    wires = [cpu.json_to_pb(desc, json.dumps({"weight": v})) for v in vals]
    dec, outs = eng.decode_batch(wires, [idx] * len(wires), mode=1)

    def ndig(s):
        m = s.split("e")[0].split("E")[0].replace(".", "").lstrip("-0")
        return len(m.rstrip("0")) or 1

    for v, r, o in zip(vals, dec, outs):
        if r["status"] != 0:
            continue  # documented host-escape boundary (near-denormal)
        text = o.decode()
        got = json.loads(text).get("weight", 0.0)
        assert float(got) == v, (v, text)
        kr = text.split(":", 1)[1].rstrip("}")
        assert ndig(kr) <= ndig(repr(v)), (v, text)


def test_parse_correctly_rounded(env):
    """encode: JSON decimal texts parse to the strtod-exact double (or the
    slot host-falls-back for the documented boundary classes)."""
    eng, cpu, desc, idx = env
    rng = random.Random(4048)

    def gen_text():
        k = rng.random()
        if k < 0.25:
            digs = "".join(rng.choices("0123456789", k=rng.randint(16, 26)))
            return f"{digs[0]}.{digs[1:]}e{rng.randint(-300, 300)}"
        if k < 0.5:
            return repr(_gen_double(rng))
        if k < 0.75:
            return f"{rng.randint(0, 10**18)}.{rng.randint(0, 10**9)}"
        return repr(rng.random() * 10 ** rng.randint(-308, 308))

    texts = [gen_text() for _ in range(20000)]
    payloads = [f'{{"weight": {t}}}'.encode() for t in texts]
    enc, pbs = eng.encode_batch(payloads, mode=1,
                                msg_indices=[idx] * len(payloads),
                                enforce=False)
    fallbacks = 0
    for t, r, w in zip(texts, enc, pbs):
        expect = float(t)
        if not math.isfinite(expect):
            continue
        if r["status"] != 0:
            fallbacks += 1  # >19-20 digits / near-DBL_MAX / near-denormal
            continue
        msg = cpu.pb_to_message(desc, w)
        assert msg.weight == expect, (t, msg.weight, expect)
    # fallbacks are the long-mantissa generator classes, not the common case
    assert fallbacks < len(texts) // 2


# ---- float32 twins -----------------------------------------------------------
# ``float`` fields take their own path (digits_roundtrip_f on decode, the
# (float) narrowing on encode); the generators and oracles are shared with
# the device twin through tests/protojson_corpus.py.

@pytest.fixture(scope="module")
def fenv():
    import protojson_corpus as pc

    return pc, pc.make_env(HostSimEngine)


def test_float32_format_shortest_roundtrip(fenv):
    pc, e = fenv
    assert pc.check_float32_format(e, seed=2025) is None


def test_float32_parse_correctly_rounded(fenv):
    pc, e = fenv
    assert pc.check_float32_parse(e, seed=4049) is None
