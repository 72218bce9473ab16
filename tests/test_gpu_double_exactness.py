"""GPU-side double exactness: the same invariants test_double_exactness
pins on the hostsim build, re-run against the REAL gfx950 kernels — a
device-codegen canary (round 2 found hipcc's fast-contract reassociating
the compensated-scaling fma chain: host exact, device off by one ulp)."""

import json
import math
import random
import struct

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from google.protobuf import descriptor_pb2

    from ggrmcp_amd.backend.discovery import ServiceDiscoverer
    from ggrmcp_amd.config import Config
    from ggrmcp_amd.engine.batch import GpuEngine
    from ggrmcp_amd.engine.cpu_ref import CpuTranscoder
    from ggrmcp_amd.utils.synthetic import synthetic_fdp

    cfg = Config.default()
    d = ServiceDiscoverer(cfg)
    fds = descriptor_pb2.FileDescriptorSet()
    fds.file.extend([synthetic_fdp()])
    d.load_descriptor_blob(fds.SerializeToString())
    eng = GpuEngine(d.tools, cfg, device=0)
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


def test_gpu_format_shortest_roundtrip(env):
    eng, cpu, desc, idx = env
    rng = random.Random(31337)
    vals = [_gen_double(rng) for _ in range(8000)]
    wires = [cpu.json_to_pb(desc, json.dumps({"weight": v})) for v in vals]
    dec, outs = [], []
    for b in range(0, len(wires), 2048):  # engine max_batch chunks
        d2, o2 = eng.decode_batch(wires[b:b + 2048],
                                  [idx] * len(wires[b:b + 2048]), mode=1)
        dec.extend(d2)
        outs.extend(o2)

    def ndig(s):
        m = s.split("e")[0].split("E")[0].replace(".", "").lstrip("-0")
        return len(m.rstrip("0")) or 1

    for v, r, o in zip(vals, dec, outs):
        if r["status"] != 0:
            continue  # documented near-denormal host escape
        text = o.decode()
        got = json.loads(text).get("weight", 0.0)
        assert float(got) == v, (v, text)
        kr = text.split(":", 1)[1].rstrip("}")
        assert ndig(kr) <= ndig(repr(v)), (v, text)


def test_gpu_parse_correctly_rounded(env):
    eng, cpu, desc, idx = env
    rng = random.Random(777)

    def gen_text():
        k = rng.random()
        if k < 0.3:
            digs = "".join(rng.choices("0123456789", k=rng.randint(16, 19)))
            return f"{digs[0]}.{digs[1:]}e{rng.randint(-250, 250)}"
        if k < 0.6:
            return repr(_gen_double(rng))
        return repr(rng.random() * 10 ** rng.randint(-300, 300))

    texts = [gen_text() for _ in range(8000)]
    payloads = [f'{{"weight": {t}}}'.encode() for t in texts]
    enc, pbs = [], []
    for b in range(0, len(payloads), 2048):
        part = payloads[b:b + 2048]
        e2, p2 = eng.encode_batch(part, mode=1, msg_indices=[idx] * len(part),
                                  enforce=False)
        enc.extend(e2)
        pbs.extend(p2)
    for t, r, w in zip(texts, enc, pbs):
        expect = float(t)
        if not math.isfinite(expect) or r["status"] != 0:
            continue
        msg = cpu.pb_to_message(desc, w)
        assert msg.weight == expect, (t, msg.weight, expect)


# ---- float32 twins (generators/oracles in tests/protojson_corpus.py) ---------

@pytest.fixture(scope="module")
def fenv():
    import protojson_corpus as pc
    from ggrmcp_amd.engine.batch import GpuEngine

    return pc, pc.make_env(lambda infos: GpuEngine(infos, device=0))


def test_gpu_float32_format_shortest_roundtrip(fenv):
    pc, e = fenv
    assert pc.check_float32_format(e, seed=31338) is None


def test_gpu_float32_parse_correctly_rounded(fenv):
    pc, e = fenv
    assert pc.check_float32_parse(e, seed=778) is None
