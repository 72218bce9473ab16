"""k_pb2json_wg with DM_UNPOPULATED / DM_STRUCTURED on gfx950.

The cases of ``tests/wg_flags_corpus.py`` through the device engine with the
routing threshold forced huge (the device's classic kernel) and low (the
workgroup kernel), byte-compared with each other and with the CPU build's
classic kernel; a mixed batch through k_tight_scan / k_compact_out; large
responses at the default threshold; and the serving pipeline with the
option on."""

import json
import random

import pytest

import protojson_corpus as pc
import unpopulated_corpus as uc
import wg_flags_corpus as wc

pytestmark = pytest.mark.gpu

FLAGS = uc.DM_UNPOPULATED | uc.DM_STRUCTURED
HUGE, LOW = "1000000000", "1"


@pytest.fixture(scope="module")
def envs():
    from ggrmcp_amd.engine.batch import GpuEngine

    return uc.make_envs(lambda infos: GpuEngine(infos, device=0))


@pytest.fixture(scope="module")
def cpu_envs():
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return uc.make_envs(HostSimEngine)


@pytest.mark.parametrize("flags", wc.FLAG_SETS)
@pytest.mark.parametrize("group", list(wc.GROUPS))
def test_gpu_groups(envs, cpu_envs, monkeypatch, group, flags):
    """One group of cases three ways: the CPU build's classic kernel, the
    device's classic kernel (threshold huge) and the workgroup kernel
    (threshold 1), all byte-identical."""
    sub = wc.GROUPS[group](envs)
    ids = list(sub)
    ref = wc.run(cpu_envs, sub, flags)
    monkeypatch.setenv("GGRMCP_WG_DEC_MIN", HUGE)
    classic = wc.run(envs, sub, flags)
    monkeypatch.setenv("GGRMCP_WG_DEC_MIN", LOW)
    coop = wc.run(envs, sub, flags)
    bad = wc.compare(sub, ref, classic, flags)
    bad += wc.compare(sub, classic, coop, flags)
    assert not bad, "\n".join(bad[:12])
    assert all(classic[c][2] == 0 for c in ids)
    routed = [c for c in ids if len(sub[c][1]) >= 1]
    assert all(coop[c][2] in (1, 2) for c in routed)
    for c in routed:
        if c in wc.OUT_OF_ORDER:
            assert coop[c][2] == 2, c
        elif group in ("sparse", "joins", "any"):
            assert coop[c][:1] + coop[c][2:3] == (0, 1), (c, coop[c][0], coop[c][2])


def test_gpu_id_shapes_at_every_alignment(envs, cpu_envs, monkeypatch):
    monkeypatch.setenv("GGRMCP_WG_DEC_MIN", LOW)
    joins = wc.chunk_joins(envs)
    wires = [w for _, w in list(joins.values())[:len(uc.ENV_IDS)]]
    s, c = envs.schema("bench.Wide64"), cpu_envs.schema("bench.Wide64")
    runs = []
    for filler in pc.WIRE_FILLERS:
        outs = uc.run_envelopes(s, envs.sink.sink_tool, [filler] + wires,
                                [0] + uc.ENV_IDS, FLAGS)
        assert outs[0][0] == 0
        runs.append(outs[1:])
    assert pc._first_diff(runs) is None
    ref = uc.run_envelopes(c, cpu_envs.sink.sink_tool,
                           [pc.WIRE_FILLERS[0]] + wires, [0] + uc.ENV_IDS, FLAGS)
    assert runs[0] == ref[1:]
    for rid, (status, out) in zip(uc.ENV_IDS, runs[0]):
        assert status == 0
        assert uc.check_envelope(out, uc.id_token(rid)) is None


def test_gpu_mixed_batch_through_compaction(envs, cpu_envs, monkeypatch):
    """Nine slots: small classic slots, routed slots, a skipped slot and a
    failing wire, so the longer envelopes go through k_tight_scan and
    k_compact_out next to classic ones."""
    monkeypatch.setenv("GGRMCP_WG_DEC_MIN", "4096")
    env = envs.sink
    s, c = envs.schema("bench.Wide64"), cpu_envs.schema("bench.Wide64")
    joins = [w for _, w in wc.chunk_joins(envs).values()]
    sparse = [w for _, w in wc.sparse_wide(envs).values()]
    small = [env.wide_cls(f01_string="k" * n).SerializeToString() for n in (3, 70)]
    wires = [small[0], joins[0], sparse[0], small[1], joins[21],
             pc.ld(1, b"bad\x80"), sparse[1], joins[5], small[0]]
    skip = [False] * 9
    skip[4] = True
    assert sum(len(w) >= 4096 for w in wires) == 5
    ids = list(range(9))
    got = uc.run_envelopes(s, env.sink_tool, wires, ids, FLAGS, skip=skip)
    ref = uc.run_envelopes(c, cpu_envs.sink.sink_tool, wires, ids, FLAGS, skip=skip)
    assert got == ref
    for i, (status, out) in enumerate(got):
        if i == 4:
            assert out is None
        elif i == 5:
            assert status == pc.E_UNSUPPORTED and out is None
        else:
            assert status == 0
            assert uc.check_envelope(out, uc.id_token(i)) is None


@pytest.mark.parametrize("target", [20_000, 64 * 1024])
def test_gpu_wide_payload_default_threshold(envs, cpu_envs, monkeypatch, target):
    """A 20 KB and a 64 KB bench.Wide64 response with both flags and the
    default threshold: the item walk answers (pad 1; the parent ran the
    classic kernel here, pad 0), the bytes are the CPU build's classic
    kernel's, the raw slice is what json_format prints."""
    from ggrmcp_amd.engine.cpu_ref import CpuTranscoder
    from ggrmcp_amd.utils.synthetic import wide_payload

    monkeypatch.delenv("GGRMCP_WG_DEC_MIN", raising=False)
    payload = wide_payload(random.Random(11), target_bytes=target)
    s = envs.schema("bench.Wide64")
    wire = CpuTranscoder().json_to_pb(s.cls.DESCRIPTOR, json.dumps(payload))
    assert len(wire) >= 16384
    cases = {"w": ("bench.Wide64", wire)}
    got = wc.run(envs, cases, FLAGS)
    ref = wc.run(cpu_envs, cases, FLAGS)
    assert not wc.compare(cases, ref, got, FLAGS)
    status, out, pad, _ = got["w"]
    assert (status, pad) == (0, 1)
    assert uc.verdict(s, wire, 0, wc.raw_slice(out), True) is None


# ---- the serving pipeline ---------------------------------------------------------

def _body(args, rid):
    return json.dumps(
        {"jsonrpc": "2.0", "id": rid, "method": "tools/call",
         "params": {"name": "bench_echoservice_echo", "arguments": args}}
    ).encode()


def _shapes():
    """The payload shapes of the workgroup decode differential test."""
    from ggrmcp_amd.utils.synthetic import wide_payload

    rng = random.Random(7)
    shapes = [wide_payload(rng, target_bytes=64 * 1024)]
    shapes.append({"attrs": {f"p{j}": "x" * 1000 for j in range(40)}})
    shapes.append({
        "f01String": ('he said "hi"\n\t\\' + "é中\U0001f600") * 20,
        "f02Int32": -7,
        "f05Bool": True,
        "items": [{"key": f"i{j}", "value": str(j), "weight": j / 3}
                  for j in range(400)],
        "attrs": {f"q{j}": "y" * 500 for j in range(20)},
    })
    shapes.append(wide_payload(rng, target_bytes=20 * 1024))
    shapes.append({
        "f01String": "a" * 1000,
        "f02Int32": 0,
        "f03Int64": "0",
        "f04Double": 1.5,
        "f05Bool": False,
        "attrs": {f"z{j}": "w" * 900 for j in range(16)},
    })
    shapes.append({
        "f01String": "p" * 1000,
        "items": [{"key": f"d{j}",
                   "value": str(rng.randint(-(2**40), 2**40)),
                   "weight": rng.random() * 10 ** rng.randint(-12, 12)}
                  for j in range(700)],
        "attrs": {f"k{j}": "v" * rng.randint(0, 40) for j in range(120)},
    })
    return shapes


@pytest.fixture()
def pipeline():
    from google.protobuf import descriptor_pb2

    from examples.protos import ALL_FDPS
    from ggrmcp_amd.backend.discovery import ServiceDiscoverer
    from ggrmcp_amd.backend.native_invoker import NativeWireClient, load_module
    from ggrmcp_amd.config import Config
    from ggrmcp_amd.engine.batch import GpuPipeline
    from ggrmcp_amd.utils.synthetic import synthetic_fdp

    srv = load_module().Server("127.0.0.1:0")
    srv.add_route("/bench.EchoService/Echo", "echo")
    bound = srv.start()
    cfg = Config.default()
    host, _, port = bound.rpartition(":")
    cfg.grpc.host, cfg.grpc.port = host, int(port)
    cfg.gpu.pinned_pool_bytes = 1 * 1024 * 1024 * 1024
    cfg.gpu.device_pool_bytes = 4 * 1024 * 1024 * 1024
    cfg.gpu.streams = 1
    d = ServiceDiscoverer(cfg)
    fdset = descriptor_pb2.FileDescriptorSet()
    fdset.file.extend(ALL_FDPS + [synthetic_fdp()])
    d.load_descriptor_blob(fdset.SerializeToString())
    d.connections[0].connect(timeout_s=15)
    wire = NativeWireClient(bound, connections=2)
    p = GpuPipeline(d, cfg, device=0, wire_clients=[wire])
    try:
        yield p
    finally:
        p.close()
        wire.close()
        d.close()
        srv.stop()


def test_gpu_pipeline_structured_routes_large_responses(pipeline, monkeypatch):
    """process_batch with the option on: classic-forced and cooperative
    bytes are equal, and only the second run routes slots to the kernel."""
    pipeline.engine.set_structured_content(True)
    bodies = [_body(a, i + 1) for i, a in enumerate(_shapes())]
    before = pipeline.engine.wg_decode_slots
    monkeypatch.setenv("GGRMCP_WG_DEC_MIN", HUGE)
    classic = pipeline.process_batch(bodies, timeout_s=30.0)
    assert pipeline.engine.wg_decode_slots == before
    monkeypatch.setenv("GGRMCP_WG_DEC_MIN", "8192")
    coop = pipeline.process_batch(bodies, timeout_s=30.0)
    assert pipeline.engine.wg_decode_slots == before + len(bodies)
    for i, (a, b) in enumerate(zip(classic, coop)):
        assert a == b, f"slot {i} diverged:\n{a[-400:]}\nvs\n{b[-400:]}"
        assert uc.check_envelope(b, str(i + 1).encode()) is None
