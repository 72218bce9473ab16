"""DM_REORDER on gfx950: ``k_pb_reorder`` over ``reorder_corpus.CASES``
against the protojson oracle and the CPU build's bytes, a mixed batch through
k_pack_out, a 20 KB slot, and ``process_batch`` with ``gpu.reorder_wire``."""

import json

import pytest

import protojson_corpus as pc
import reorder_corpus as rc
import unpopulated_corpus as uc
import wg_flags_corpus as wc
from protojson_corpus import ld

pytestmark = pytest.mark.gpu

RO, MODES = rc.RO, rc.MODES


@pytest.fixture(scope="module")
def envs():
    from ggrmcp_amd.engine.batch import GpuEngine

    return rc.make_envs(lambda infos: GpuEngine(infos, device=0))


@pytest.fixture(scope="module")
def cpu_envs():
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return rc.make_envs(lambda infos: HostSimEngine(infos, wg=True))


@pytest.fixture(scope="module")
def answers(envs, cpu_envs):
    ids = list(rc.CASES)
    return {m: (rc.run(envs, ids, m), rc.run(cpu_envs, ids, m)) for m in MODES}


@pytest.mark.parametrize("cid", list(rc.CASES))
def test_case(envs, answers, cid):
    """The oracle's value and the CPU build's bytes; refused with the flag clear."""
    for m in MODES:
        gpu, cpu = answers[m]
        assert rc.judge(envs, cid, m, gpu[cid]) is None, (cid, m)
        assert gpu[cid] == cpu[cid], (cid, m)
    st, _, pad, _ = rc.run(envs, [cid], 1)[cid]
    assert st != 0 and pad == 0


@pytest.mark.parametrize("flags", wc.FLAG_SETS)
def test_in_order_wires_do_not_move(envs, flags):
    cases = wc.all_cases(envs.base)
    off, on = wc.run(envs.base, cases, flags), wc.run(envs.base, cases, flags | RO)
    same = [c for c in cases if off[c][0] == 0]
    assert len(same) > 100 and all(off[c][:3] == on[c][:3] for c in same)


def test_mixed_batch_through_pack_out(envs):
    s = envs.schema("x.Rich")   # in-order, reordered, skipped, gave-up, reordered
    names = [None, "swap-top", None, "runs-max+1", "message-merge"]
    wires = [rc.CASES[n][1] if n else ld(14, b"in-order") for n in names]
    wires[2] = None
    before = s.engine.reorder_slots
    dec, outs = s.engine.decode_batch(wires, [s.idx] * 5, mode=1 | RO)
    assert s.engine._eng.compact_used
    assert [int(r["status"]) for r in dec] == [0, 0, 0, pc.E_UNSUPPORTED, 0]
    assert [int(r["pad"]) for r in dec] == [0, 3, 0, 0, 3]
    offs = [int(r["out_off"]) for r in dec]
    assert offs == sorted(offs) and offs[1] > offs[0] and offs[4] > offs[1]
    assert s.engine.reorder_slots == before + 2
    for i in (0, 1, 4):
        assert uc.verdict(s, wires[i], 0, outs[i], False) is None, i


def test_20k_wide64_at_the_default_threshold(envs):
    """attrs ahead of a 20 KB f01_string: refused by k_pb2json_wg."""
    s = envs.schema("bench.Wide64")
    wire = (s.cls(attrs={"k": "v"}).SerializeToString()
            + s.cls(f01_string="s" * 20_000).SerializeToString())
    enc, _ = s.engine.encode_batch(
        uc.envelope_bodies(envs.tool("bench.Wide64"), [7]), mode=0)
    assert int(enc[0]["status"]) == 0
    dec, outs = s.engine.decode_batch([wire], [s.idx], mode=0 | RO)
    assert (int(dec[0]["status"]), int(dec[0]["pad"])) == (0, 3)
    text = pc.loads(outs[0].decode())["result"]["content"][0]["text"]
    assert uc.verdict(s, wire, 0, text.encode(), False) is None


@pytest.fixture(scope="module")
def echo():
    from google.protobuf import descriptor_pb2

    from examples.protos import ALL_FDPS
    from ggrmcp_amd.backend.discovery import ServiceDiscoverer
    from ggrmcp_amd.backend.native_invoker import NativeWireClient, load_module
    from ggrmcp_amd.config import Config
    from ggrmcp_amd.utils.synthetic import synthetic_fdp

    srv = load_module().Server("127.0.0.1:0")
    srv.add_route("/bench.EchoService/Echo", "echo")
    bound = srv.start()
    cfg = Config.default()
    cfg.grpc.host, cfg.grpc.port = bound.rpartition(":")[0], int(bound.rpartition(":")[2])
    cfg.gpu.streams, cfg.gpu.reorder_wire = 1, True
    d = ServiceDiscoverer(cfg)
    d.load_descriptor_blob(descriptor_pb2.FileDescriptorSet(
        file=ALL_FDPS + [synthetic_fdp()]).SerializeToString())
    d.connections[0].connect(timeout_s=15)
    wire = NativeWireClient(bound, connections=2)
    yield d, cfg, wire
    wire.close()
    d.close()
    srv.stop()


@pytest.mark.parametrize("native", [True, False], ids=["native-span", "grpcio-span"])
def test_process_batch_with_reorder_wire(echo, native):
    """Out-of-order arguments echoed back as out-of-order wire, both spans."""
    from ggrmcp_amd.engine.batch import GpuPipeline

    d, cfg, wire = echo
    pipeline = GpuPipeline(d, cfg, device=0, wire_clients=[wire] if native else None)
    eng, mi = pipeline.engine, d.tools["bench_echoservice_echo"]
    args = {"attrs": {"k": "v"}, "f02Int32": 5, "f01String": "a"}
    body = json.dumps({"jsonrpc": "2.0", "id": 9, "method": "tools/call",
                       "params": {"name": "bench_echoservice_echo",
                                  "arguments": args}}).encode()
    want = json.loads(pipeline.cpu.pb_to_json(
        mi.output_descriptor,
        pipeline.cpu.json_to_pb(mi.input_descriptor, json.dumps(args))))

    def call():
        resp = json.loads(pipeline.process_batch([body], timeout_s=30.0)[0])
        assert resp["id"] == 9 and resp["result"]["isError"] is False, resp
        return json.loads(resp["result"]["content"][0]["text"])

    falls, slots = eng.stats.host_fallbacks, eng.reorder_slots
    assert call() == want
    assert (eng.stats.host_fallbacks, eng.reorder_slots) == (falls, slots + 1)
    eng.set_reorder_wire(False)
    assert call() == want
    assert (eng.stats.host_fallbacks, eng.reorder_slots) == (falls + 1, slots + 1)
