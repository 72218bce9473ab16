"""DM_UNPOPULATED / DM_STRUCTURED on gfx950: the corpus and targeted cases of
``tests/unpopulated_corpus.py`` on the device engine, the structured
envelope at every slot alignment and through k_tight_scan/k_compact_out,
byte-compared with the CPU build of the same kernel source, and the option
end to end through the native frontend."""

import contextlib
import http.client
import json
import random

import pytest

import protojson_corpus as pc
import unpopulated_corpus as uc

pytestmark = pytest.mark.gpu

FLAGS = uc.DM_UNPOPULATED | uc.DM_STRUCTURED
TARGETED = uc.targeted_cases(uc.sink_descriptor())


@pytest.fixture(scope="module")
def envs():
    from ggrmcp_amd.engine.batch import GpuEngine

    return uc.make_envs(lambda infos: GpuEngine(infos, device=0))


@pytest.fixture(scope="module")
def cpu_envs():
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return uc.make_envs(HostSimEngine)


@pytest.fixture(scope="module")
def corpus(envs):
    return uc.run_corpus(envs)


def test_gpu_flag_adds_no_host_escape(corpus):
    clear = {i for i, (a, _) in corpus.items() if a == "host"}
    flagged = {i for i, (_, b) in corpus.items() if b == "host"}
    assert flagged == clear, sorted(flagged ^ clear)


@pytest.mark.parametrize("case_id", uc.corpus_ids())
def test_gpu_corpus_wire(corpus, case_id):
    clear, flagged = corpus[case_id]
    assert clear in (None, "host"), f"flag clear: {clear}"
    assert flagged in (None, "host"), f"DM_UNPOPULATED: {flagged}"
    assert (flagged == "host") == (clear == "host")


def test_gpu_targeted(envs, cpu_envs):
    """Every targeted case in one batch per schema: status and value as the
    oracle says, and the text byte-identical to the CPU build's."""
    by_schema = {}
    for cid, (name, wire, expected) in TARGETED.items():
        by_schema.setdefault(name, []).append((cid, wire, expected))
    name, wire = uc.expansion_case()
    by_schema.setdefault(name, []).append(("expansion", wire, "ok-or-overflow"))
    bad = []
    for name, cases in by_schema.items():
        s, c = envs.schema(name), cpu_envs.schema(name)
        wires = [w for _, w, _ in cases]
        got = uc.decode(s, wires, uc.DM_UNPOPULATED)
        ref = uc.decode(c, wires, uc.DM_UNPOPULATED)
        for (cid, w, expected), (st, out), (cst, cout) in zip(cases, got, ref):
            if (st, out) != (cst, cout):
                bad.append(f"{cid}: device {st} {out!r} != cpu build {cst} {cout!r}")
            elif expected == "ok-or-overflow" and st == pc.E_OVERFLOW:
                continue
            elif expected in ("ok", "ok-or-overflow"):
                why = uc.verdict(s, w, st, out, True)
                if st != 0 or why is not None:
                    bad.append(f"{cid}: status {st} {why}")
            elif st != expected:
                bad.append(f"{cid}: status {st}, want {expected}")
    assert not bad, "\n".join(bad)


def _sweep_inputs(env):
    strings = uc.envelope_strings()
    wires = [env.inner_cls(key=t).SerializeToString() for t in strings]
    ids = [uc.ENV_IDS[i % len(uc.ENV_IDS)] for i in range(len(wires))]
    return strings, wires, ids


def test_gpu_envelope_sweep_all_alignments(envs, cpu_envs):
    """The string sweep of the CPU envelope test behind a leading filler
    slot one byte longer each run: every slot start at every residue mod 4,
    results byte-identical across runs and to the CPU build."""
    env = envs.sink
    s, c = envs.schema("bench.Inner"), cpu_envs.schema("bench.Inner")
    strings, wires, ids = _sweep_inputs(env)
    runs = []
    for filler in pc.WIRE_FILLERS:
        outs = uc.run_envelopes(s, env.sink_tool, [filler] + wires, [0] + ids, FLAGS)
        assert outs[0][0] == 0, "filler slot"
        runs.append(outs[1:])
    assert pc._first_diff(runs) is None
    ref = uc.run_envelopes(c, cpu_envs.sink.sink_tool, [pc.WIRE_FILLERS[0]] + wires,
                           [0] + ids, FLAGS)[1:]
    assert runs[0] == ref
    for k, (status, out) in enumerate(runs[0]):
        assert status == 0, (k, status)
        why = uc.check_envelope(out, uc.id_token(ids[k]))
        assert why is None, (k, why)
        assert json.loads(out)["result"]["structuredContent"]["key"] == strings[k]


@pytest.mark.parametrize("n", [1, 255, 257])
def test_gpu_structured_compaction(envs, cpu_envs, n):
    """Every fifth slot skipped, every seventh a failing wire: the longer
    envelopes through k_tight_scan / k_compact_out equal the CPU build's."""
    env = envs.sink
    s, c = envs.schema("bench.Inner"), cpu_envs.schema("bench.Inner")
    wires, skip = [], []
    for i in range(n):
        if n > 1 and i % 7 == 3:
            wires.append(pc.ld(1, b"bad\x80"))
        else:
            wires.append(env.inner_cls(key="k" * (i % 70), value=i).SerializeToString())
        skip.append(n > 1 and i % 5 == 4)
    ids = list(range(n))
    got = uc.run_envelopes(s, env.sink_tool, wires, ids, FLAGS, skip=skip)
    ref = uc.run_envelopes(c, cpu_envs.sink.sink_tool, wires, ids, FLAGS, skip=skip)
    assert got == ref
    for i, (status, out) in enumerate(got):
        if skip[i]:
            assert out is None
        elif n > 1 and i % 7 == 3:
            assert status == pc.E_UNSUPPORTED and out is None
        else:
            assert status == 0
            assert uc.check_envelope(out, uc.id_token(i)) is None


def test_gpu_wide64_20k_structured(envs, cpu_envs):
    """One 20 KB bench.Wide64 response with both flags: above the workgroup
    kernel's threshold, so it runs the classic kernel.  Correct against the
    oracle and byte-identical to the CPU build."""
    from ggrmcp_amd.engine.cpu_ref import CpuTranscoder
    from ggrmcp_amd.utils.synthetic import wide_payload

    env = envs.sink
    s, c = envs.schema("bench.Wide64"), cpu_envs.schema("bench.Wide64")
    payload = wide_payload(random.Random(11), target_bytes=20000)
    wire = CpuTranscoder().json_to_pb(s.cls.DESCRIPTOR, json.dumps(payload))
    assert len(wire) >= 16384
    (status, out), = uc.run_envelopes(s, env.sink_tool, [wire], ["w"], FLAGS)
    (cst, cout), = uc.run_envelopes(c, cpu_envs.sink.sink_tool, [wire], ["w"], FLAGS)
    assert status == 0 and (status, out) == (cst, cout)
    assert uc.check_envelope(out, b'"w"') is None
    raw = out[out.rfind(uc.P_STRUCT) + len(uc.P_STRUCT):-len(uc.P_TAIL)]
    assert uc.verdict(s, wire, 0, raw, True) is None


# ---- end to end through the native frontend ------------------------------------

@contextlib.contextmanager
def _gateway(structured):
    from google.protobuf import descriptor_pb2

    from examples.protos import ALL_FDPS
    from ggrmcp_amd.backend.discovery import ServiceDiscoverer
    from ggrmcp_amd.backend.native_invoker import NativeWireClient, load_module
    from ggrmcp_amd.config import Config
    from ggrmcp_amd.engine.batch import GpuPipeline
    from ggrmcp_amd.server.native_http import NativeHTTPGateway

    srv = load_module().Server("127.0.0.1:0")
    # SayHello answered by the echo route: the reply wire is the request
    # wire, and HelloRequest.name shares field 1 with HelloResponse.message,
    # so an empty name gives an EMPTY reply
    srv.add_route("/hello.HelloService/SayHello", "echo")
    bound = srv.start()
    cfg = Config.default()
    host, _, port = bound.rpartition(":")
    cfg.grpc.host, cfg.grpc.port = host, int(port)
    cfg.server.rate_limit_rps = 1_000_000
    cfg.server.rate_limit_burst = 1_000_000
    cfg.server.structured_content = structured
    cfg.gpu.streams = 1
    d = ServiceDiscoverer(cfg)
    fdset = descriptor_pb2.FileDescriptorSet()
    fdset.file.extend(ALL_FDPS)
    d.load_descriptor_blob(fdset.SerializeToString())
    d.connections[0].connect(timeout_s=15)
    wire = NativeWireClient(bound, connections=2)
    pipeline = GpuPipeline(d, cfg, device=0, wire_clients=[wire])
    gw = NativeHTTPGateway(pipeline, d, cfg)
    port_http = gw.start()
    try:
        yield gw, port_http, pipeline
    finally:
        gw.stop()
        wire.close()
        d.close()
        srv.stop()


def _post(port, payload):
    conn = http.client.HTTPConnection("127.0.0.1", port, timeout=15)
    conn.request("POST", "/", body=json.dumps(payload),
                 headers={"Content-Type": "application/json"})
    r = conn.getresponse()
    data = r.read()
    conn.close()
    return r.status, data


def _hello(rid, name):
    return {"jsonrpc": "2.0", "id": rid, "method": "tools/call",
            "params": {"name": "hello_helloservice_sayhello",
                       "arguments": {"name": name}}}


def test_gpu_serving_with_the_option_on():
    with _gateway(True) as (gw, port, pipeline):
        assert gw._span_engines, "the span executor must be live"
        st0 = gw._fe.native_stats()
        status, empty = _post(port, _hello(1, ""))
        assert status == 200
        assert empty == (b'{"jsonrpc":"2.0","id":1,"result":{"content":[{"type":'
                         b'"text","text":"{\\"message\\":\\"\\"}"}],'
                         b'"structuredContent":{"message":""},"isError":false}}')
        status, full = _post(port, _hello("two", 'a"b'))
        assert status == 200
        assert uc.check_envelope(full, b'"two"') is None
        assert json.loads(full)["result"]["structuredContent"] == {"message": 'a"b'}
        st1 = gw._fe.native_stats()
        assert st1["gpuOk"] - st0["gpuOk"] == 2
        assert pipeline.engine.stats.snapshot()["hostFallbacks"] == 0


def test_gpu_serving_with_the_option_off():
    with _gateway(False) as (gw, port, pipeline):
        assert gw._span_engines
        status, body = _post(port, _hello(1, ""))
        assert status == 200
        assert body == (b'{"jsonrpc":"2.0","id":1,"result":{"content":[{"type":'
                        b'"text","text":"{}"}],"isError":false}}')
        assert pipeline.engine.stats.snapshot()["hostFallbacks"] == 0
