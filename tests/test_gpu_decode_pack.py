"""The decode tail on gfx950: k_pack_out writes the packed bytes and the
results into pinned host memory itself, and the encode D2H span ends at the
live pb bytes (the pb base moves with the batch size).

Every batch is also run through the CPU build of the decode kernels
(HostSimEngine); statuses, lengths and bytes must be equal, and each slot's
bytes must start at the Python prefix sum of the aligned lengths before it."""

import json
import random

import pytest
from google.protobuf import message_factory

import protojson_corpus as pc
import unpopulated_corpus as uc

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 255, 256, 257, 513)
TRUNCATED = b"\x0a\x05ab"   # field 1, five bytes announced, two present


class Env:
    def __init__(self, gpu_factory):
        from examples.protos import ALL_FDPS
        from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos
        from ggrmcp_amd.engine.hostsim import HostSimEngine

        fdps = ALL_FDPS + [pc.sink_fdp()]
        self.pool = build_pool(fdps)
        self.infos = {m.tool_name(): m for m in
                      extract_method_infos(fdps, self.pool, compat_names=False)}
        self.cpu = HostSimEngine(self.infos)
        self.gpu = gpu_factory(self.infos)
        self.hello_tool = next(
            n for n, mi in self.infos.items()
            if mi.input_descriptor.full_name == "hello.HelloRequest")
        self.hello = self.cls("hello.HelloResponse")
        self.sink = self.cls("t.Sink")
        idx = self.cpu.tables.msg_index
        self.hello_idx, self.sink_idx = idx["hello.HelloResponse"], idx["t.Sink"]

    def cls(self, name):
        return message_factory.GetMessageClass(
            self.pool.FindMessageTypeByName(name))


@pytest.fixture(scope="module")
def env():
    from ggrmcp_amd.engine.batch import GpuEngine

    return Env(lambda infos: GpuEngine(infos, device=0))


def batch(env, n, all_skipped=False):
    """n slots of hello and t.Sink responses, 0-300 bytes of wire, whose JSON
    lengths walk through every residue mod 4; every eleventh wire is
    truncated; the first, middle and last slots are skipped (n >= 3)."""
    wires, idx = [], []
    for i in range(n):
        if i % 11 == 5:
            w = TRUNCATED
        elif i % 13 == 7:
            w = b""
        elif i % 2 == 0:
            w = env.hello(message="m" * ((i * 7) % 297)).SerializeToString()
        else:
            w = env.sink(snake_case_field="s" * ((i * 5) % 290),
                         opt_i32=i).SerializeToString()
        assert len(w) <= 300
        wires.append(w)
        idx.append(env.hello_idx if i % 2 == 0 else env.sink_idx)
    skip = [all_skipped or (n >= 3 and i in (0, n // 2, n - 1))
            for i in range(n)]
    return wires, idx, skip


def run(env, engine, wires, idx, skip, mode):
    if (mode & 3) == 0:
        enc, _ = engine.encode_batch(
            uc.envelope_bodies(env.hello_tool, list(range(len(wires)))), mode=0)
        assert all(int(r["status"]) == 0 for r in enc)
    return engine.decode_batch(wires, idx, mode=mode, skip=skip)


def compare(env, wires, idx, skip, mode, packed=True):
    ref_dec, ref_out = run(env, env.cpu, wires, idx, skip, mode)
    dec, out = run(env, env.gpu, wires, idx, skip, mode)
    assert dec["status"].tolist() == ref_dec["status"].tolist()
    assert dec["out_len"].tolist() == ref_dec["out_len"].tolist()
    assert out == ref_out
    assert bool(env.gpu._eng.compact_used) is packed
    if packed:
        acc, want = 0, []
        for n in ref_dec["out_len"].tolist():
            want.append(acc)
            acc += (n + 3) & ~3
        assert dec["out_off"].tolist() == want
    return ref_dec, ref_out


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("n", SIZES)
def test_gpu_packed_batches(env, n, mode):
    wires, idx, skip = batch(env, n)
    dec, out = compare(env, wires, idx, skip, mode)
    live = [i for i in range(n) if not skip[i] and wires[i] != TRUNCATED]
    assert all(int(dec[i]["status"]) == 0 and out[i] for i in live)
    assert all(int(dec[i]["status"]) != 0 for i in range(n)
               if wires[i] == TRUNCATED and not skip[i])
    if n >= 255:
        assert {len(out[i]) % 4 for i in live} == {0, 1, 2, 3}


@pytest.mark.parametrize("n", [1, 2, 257])
def test_gpu_all_skipped(env, n):
    wires, idx, skip = batch(env, n, all_skipped=True)
    dec, out = compare(env, wires, idx, skip, 1)
    assert out == [None] * n and not dec["out_len"].any()


def test_gpu_no_stale_results(env):
    """257 slots, then 2 on the same engine: the second answer holds nothing
    of the first."""
    compare(env, *batch(env, 257), 1)
    wires, idx, _ = batch(env, 2)
    dec, out = compare(env, wires, idx, [False, False], 1)
    assert [json.loads(o) for o in out] == [
        {}, {"optI32": 1, "snakeCaseField": "sssss"}]


def test_gpu_overflow_takes_the_arena_copy():
    """cap_pb (4 KB) below one batch's packed output (about 10 KB of \\u0001
    escapes): the answers equal the CPU build's and come from the arena copy;
    a batch that fits is packed again afterwards."""
    from ggrmcp_amd.config import Config
    from ggrmcp_amd.engine.batch import GpuEngine

    cfg = Config.default()
    cfg.gpu.pinned_pool_bytes = 16 * 1024   # cap_in = cap_pb = 4 KB
    cfg.gpu.device_pool_bytes = 1024 * 1024
    small = Env(lambda infos: GpuEngine(infos, cfg, device=0))
    wires = [small.hello(message="\x01" * (96 + i)).SerializeToString()
             for i in range(16)]
    assert sum(map(len, wires)) < 4096
    idx = [small.hello_idx] * 16
    dec, out = compare(small, wires, idx, [False] * 16, 1, packed=False)
    assert sum((len(o) + 3) & ~3 for o in out) > 4096
    assert all(json.loads(o)["message"] == "\x01" * (96 + i)
               for i, o in enumerate(out))
    compare(small, wires[:4], idx[:4], [False] * 4, 1, packed=True)


@pytest.mark.parametrize("n", [1, 61, 257])
def test_gpu_encode_base_follows_the_batch(env, n):
    """Encode n bodies (results, ids and pb wire against the CPU build), then
    decode on the same engine with no encode in between: the envelopes replay
    the ids, and the packed bytes land at the base the encode left."""
    from ggrmcp_amd.utils.synthetic import hello_payload, jsonrpc_body

    rng = random.Random(n)
    bodies = [jsonrpc_body(env.hello_tool, hello_payload(rng, 40 + 17 * (i % 60)),
                           f"id-{i}" if i % 3 else i)
              for i in range(n)]
    ref_enc, ref_pb = env.cpu.encode_batch(bodies, mode=0)
    enc, pb = env.gpu.encode_batch(bodies, mode=0)
    assert enc.tobytes() == ref_enc.tobytes()
    assert pb == ref_pb and all(pb)
    wires = [env.hello(message=f"Hello, {i}!" + "x" * (i % 50)).SerializeToString()
             for i in range(n)]
    idx, skip = [env.hello_idx] * n, [False] * n
    ref_dec, ref_out = env.cpu.decode_batch(wires, idx, mode=0, skip=skip)
    for _ in range(2):   # the second decode has no encode before it either
        dec, out = env.gpu.decode_batch(wires, idx, mode=0, skip=skip)
        assert dec["status"].tolist() == ref_dec["status"].tolist() == [0] * n
        assert out == ref_out
        assert env.gpu._eng.compact_used
    for i in (0, n // 2, n - 1):
        resp = json.loads(out[i])
        assert resp["id"] == (f"id-{i}" if i % 3 else i)
        assert json.loads(resp["result"]["content"][0]["text"])["message"] \
            .startswith(f"Hello, {i}!")


def test_gpu_forced_workgroup_slots_share_the_tail(env, monkeypatch):
    """Threshold forced low: two slots go to k_pb2json_wg and pass through
    k_pack_out next to two classic ones."""
    monkeypatch.setenv("GGRMCP_WG_DEC_MIN", "64")
    wires = [env.hello(message="a").SerializeToString(),
             env.hello(message="b" * 203).SerializeToString(),
             env.sink(snake_case_field="c" * 281, opt_i32=3).SerializeToString(),
             env.sink(opt_i32=4).SerializeToString()]
    idx = [env.hello_idx, env.hello_idx, env.sink_idx, env.sink_idx]
    before = env.gpu.wg_decode_slots
    compare(env, wires, idx, [False] * 4, 0)
    assert env.gpu.wg_decode_slots == before + 2


def test_gpu_process_batch_end_to_end():
    """61 SayHello calls through the pipeline: encode, invoke, decode."""
    from examples.bench_backend import serve
    from ggrmcp_amd.backend.discovery import ServiceDiscoverer
    from ggrmcp_amd.backend.native_invoker import NativeWireClient
    from ggrmcp_amd.config import Config
    from ggrmcp_amd.engine.batch import GpuPipeline
    from ggrmcp_amd.utils.synthetic import jsonrpc_body

    server, target = serve("127.0.0.1:0")
    d = wire = pipeline = None
    try:
        cfg = Config.default()
        host, _, port = target.rpartition(":")
        cfg.grpc.host, cfg.grpc.port = host, int(port)
        d = ServiceDiscoverer(cfg)
        d.connect(timeout_s=30)
        d.discover()
        wire = NativeWireClient(target, connections=2)
        pipeline = GpuPipeline(d, cfg, device=0, wire_clients=[wire])
        names = ["n" * (1 + (i * 37) % 300) + str(i) for i in range(61)]
        bodies = [jsonrpc_body("hello_helloservice_sayhello", {"name": nm}, i)
                  for i, nm in enumerate(names)]
        for _ in range(2):
            out = pipeline.process_batch(bodies, timeout_s=30.0)
            assert len(out) == 61
            for i, o in enumerate(out):
                resp = json.loads(o)
                assert resp["id"] == i and resp["result"]["isError"] is False
                inner = json.loads(resp["result"]["content"][0]["text"])
                assert inner["message"].startswith("Hello, ")
                assert names[i] in inner["message"]
        assert pipeline.engine.stats.snapshot()["gpuOk"] == 122
    finally:
        if pipeline is not None:
            pipeline.close()
        if wire is not None:
            wire.close()
        if d is not None:
            d.close()
        server.stop(grace=None)
