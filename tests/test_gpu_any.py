"""google.protobuf.Any on gfx950: the corpus of tests/any_corpus.py through
the real 64-lane kernels (one launch per list), the URL-length sweep at all
four slot alignments (the name hash and its byte compare straddle lane
windows there, which the single-lane CPU build cannot judge), classic vs
workgroup kernels byte for byte, and the serving pipeline end to end."""

import json
import os

import pytest
from google.protobuf import json_format

import any_corpus as ac
import protojson_corpus as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from ggrmcp_amd.engine.batch import GpuEngine

    return ac.make_env(lambda infos: GpuEngine(infos, device=0))


@pytest.fixture(scope="module")
def wires(env):
    return ac.accept_wires(env)


def _report(res):
    bad = {k: v for k, v in res.items() if v}
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())


def test_gpu_any_encode(env):
    _report(ac.run_encode(env, ac.ACCEPT))
    _report(ac.run_encode(env, ac.REJECT + ac.ORACLE_DECIDES))
    # the device-handled shapes are answered by the device, not the host
    plain = [c for c in ac.ACCEPT if not c.host]
    enc, _ = env.engine.encode_batch([c.data.encode() for c in plain], mode=1,
                                     msg_indices=[env.idx] * len(plain),
                                     enforce=False)
    assert [c.id for c, r in zip(plain, enc) if int(r["status"])] == []


def test_gpu_any_decode(env, wires):
    _report(ac.run_decode(env, ac.ACCEPT, wires, mode=1))
    _report(ac.run_decode(env, ac.WIRES, [c.data for c in ac.WIRES], mode=1))
    # the untagged shapes are answered by the device, not the host
    dec, _ = env.engine.decode_batch(list(wires), [env.idx] * len(wires), mode=1)
    assert [c.id for c, r in zip(ac.ACCEPT, dec)
            if int(r["status"]) and not c.host] == []


def test_gpu_any_decode_envelope(env, wires):
    _report(ac.run_decode(env, ac.ACCEPT, wires, mode=0))
    _report(ac.run_decode(env, ac.WIRES, [c.data for c in ac.WIRES], mode=0))


def test_gpu_any_url_sweep_at_four_alignments(env):
    """URLs of 62-66 and 254-258 bytes behind a leading filler slot one byte
    longer each run: every slot start visits each residue mod 4, and the
    results are byte-identical across the runs and right by the oracle."""
    cases = [c for c in ac.ACCEPT if c.id.startswith("url-len-")]
    assert len(cases) == len(ac.URL_LENGTHS)
    n = len(cases) + 1
    runs = []
    for fl in pc.JSON_FILLERS:
        enc, pbs = env.engine.encode_batch(
            [fl] + [c.data.encode() for c in cases], mode=1,
            msg_indices=[env.idx] * n, enforce=False)
        assert int(enc[0]["status"]) == 0, "filler slot"
        _report(ac.encode_verdicts(env, cases, enc[1:], pbs[1:]))
        runs.append([(int(r["status"]), pb) for r, pb in zip(enc[1:], pbs[1:])])
    assert pc._first_diff(runs) is None, pc._first_diff(runs)
    # URLs up to 256 bytes are resolved on the device
    assert [st for st, _ in runs[0]] == [0] * 8 + [6, 6]

    ws = [json_format.Parse(c.data, env.cls(), descriptor_pool=env.pool)
          .SerializeToString() for c in cases]
    runs = []
    for k in range(1, 5):
        dec, outs = env.engine.decode_batch(
            [ac.ld(4, b"x" * k)] + ws, [env.idx] * n, mode=1)
        assert int(dec[0]["status"]) == 0, "filler slot"
        _report(ac.decode_verdicts(env, cases, ws, dec[1:], outs[1:], lambda o: o))
        runs.append([(int(r["status"]), o) for r, o in zip(dec[1:], outs[1:])])
    assert pc._first_diff(runs) is None, pc._first_diff(runs)
    assert [st for st, _ in runs[0]] == [0] * len(cases)


# ---- serving pipeline: workgroup kernels and end to end ----------------------

@pytest.fixture(scope="module")
def served():
    from google.protobuf import descriptor_pb2

    from ggrmcp_amd.backend.discovery import ServiceDiscoverer
    from ggrmcp_amd.backend.native_invoker import NativeWireClient, load_module
    from ggrmcp_amd.config import Config
    from ggrmcp_amd.engine.batch import GpuPipeline

    srv = load_module().Server("127.0.0.1:0")
    srv.add_route("/t.AnyService/Echo", "echo")
    bound = srv.start()
    cfg = Config.default()
    host, _, port = bound.rpartition(":")
    cfg.grpc.host, cfg.grpc.port = host, int(port)
    cfg.gpu.streams = 1
    d = ServiceDiscoverer(cfg)
    fdset = descriptor_pb2.FileDescriptorSet()
    fdset.file.extend([ac.other_fdp(), ac.anyh_fdp()])
    d.load_descriptor_blob(fdset.SerializeToString())
    d.connections[0].connect(timeout_s=15)
    wire = NativeWireClient(bound, connections=2)
    pipeline = GpuPipeline(d, cfg, device=0, wire_clients=[wire])
    tool = next(n for n in d.tools if n.endswith("echo"))
    yield pipeline, d, tool
    os.environ.pop("GGRMCP_WG_ENC_MIN", None)
    os.environ.pop("GGRMCP_WG_DEC_MIN", None)
    wire.close()
    d.close()
    srv.stop()


def _body(tool, args, rid):
    return json.dumps({"jsonrpc": "2.0", "id": rid, "method": "tools/call",
                       "params": {"name": tool, "arguments": args}}).encode()


def _big_shapes():
    """~10 KB runs of 48 Any entries of ~200 bytes each."""
    def entry(j):
        if j % 5 == 3:
            return {"@type": ac.TG + "google.protobuf.StringValue",
                    "value": "s" * (150 + j % 7)}
        if j % 5 == 4:
            return {"@type": ac.TG + "u.Other", "d": [j + 0.5] * 12}
        return {"@type": ac.TG + "t.Leaf", "id": j + 1, "tag": "y" * (140 + j % 9)}

    ra = {"ra": [entry(j) for j in range(48)], "after": "z"}
    ma = {"ma": {f"k{j:02d}": entry(j) for j in range(48)}, "after": "z"}
    both = {"a": ac.LEAF, "ra": ra["ra"][:24], "ma": ma["ma"], "oa": entry(4)}
    return [ra, ma, both]


def _answers_match(pipeline, d, tool, shapes, out):
    mi = d.tools[tool]
    pool = mi.input_descriptor.file.pool
    for i, (args, raw) in enumerate(zip(shapes, out)):
        resp = json.loads(raw)
        assert resp["id"] == i + 1
        assert resp["result"]["isError"] is False, resp
        inner = pc.loads(resp["result"]["content"][0]["text"])
        wire = pipeline.cpu.json_to_pb(mi.input_descriptor, json.dumps(args))
        oracle = pc.loads(pipeline.cpu.pb_to_json(mi.output_descriptor, wire))
        assert ac.same_json(inner, oracle, mi.output_descriptor, pool), \
            f"slot {i}:\nkernel: {inner}\noracle: {oracle}"


def test_gpu_any_wg_encode_matches_classic_bytes(served):
    pipeline, d, tool = served
    bodies = [_body(tool, a, i + 1) for i, a in enumerate(_big_shapes())]
    assert all(9000 < len(b) < 40000 for b in bodies)
    try:
        os.environ["GGRMCP_WG_ENC_MIN"] = "1000000000"     # force classic
        enc_a, pbs_a = pipeline.engine.encode_batch(bodies, mode=0)
        os.environ["GGRMCP_WG_ENC_MIN"] = "2048"           # force cooperative
        enc_b, pbs_b = pipeline.engine.encode_batch(bodies, mode=0)
    finally:
        os.environ.pop("GGRMCP_WG_ENC_MIN", None)
    for i in range(len(bodies)):
        assert int(enc_a[i]["status"]) == 0 == int(enc_b[i]["status"]), i
        assert pbs_a[i] == pbs_b[i], f"slot {i} wire diverged"


def test_gpu_any_wg_decode_matches_classic_bytes(served):
    pipeline, d, tool = served
    shapes = _big_shapes()
    bodies = [_body(tool, a, i + 1) for i, a in enumerate(shapes)]
    before = pipeline.engine.stats.host_fallbacks
    try:
        os.environ["GGRMCP_WG_DEC_MIN"] = "1000000000"     # force classic
        classic = pipeline.process_batch(bodies, timeout_s=30.0)
        os.environ["GGRMCP_WG_DEC_MIN"] = "2048"           # force cooperative
        coop = pipeline.process_batch(bodies, timeout_s=30.0)
    finally:
        os.environ.pop("GGRMCP_WG_DEC_MIN", None)
    for i, (a, b) in enumerate(zip(classic, coop)):
        assert a == b, f"slot {i} diverged:\n{a[:400]}\nvs\n{b[:400]}"
    _answers_match(pipeline, d, tool, shapes, coop)
    assert pipeline.engine.stats.host_fallbacks == before


def test_gpu_any_end_to_end(served):
    """32 device-handled bodies: right answers, hostFallbacks does not move.
    Then "@type" second: the right answer again, through exactly one host
    fallback — the host path resolves the backend's types too."""
    pipeline, d, tool = served
    # the echoed wire keeps the JSON member order, and out-of-order wire
    # fields are an older host-escape rule of the decode kernel: these three
    # corpus shapes list a higher field number first, so a field-ordered
    # three-deep shape stands in for them
    unordered = {"any-last", "deep-3", "deep-next"}
    shapes = [json.loads(c.data) for c in ac.ACCEPT
              if not c.host and c.id not in unordered][:31]
    shapes.append({"a": {"@type": "t.Deep", "inner": {
        "@type": "t.Deep", "inner": {"@type": "t.Deep", "inner": ac.LEAF,
                                     "s": "3"}, "s": "2"}, "s": "1"},
        "after": "z"})
    assert len(shapes) == 32
    bodies = [_body(tool, a, i + 1) for i, a in enumerate(shapes)]
    before = pipeline.engine.stats.snapshot()["hostFallbacks"]
    out = pipeline.process_batch(bodies, timeout_s=30.0)
    _answers_match(pipeline, d, tool, shapes, out)
    assert pipeline.engine.stats.snapshot()["hostFallbacks"] == before

    second = {"a": {"id": 5, "tag": "x", "@type": ac.TG + "t.Leaf"}, "after": "z"}
    out = pipeline.process_batch([_body(tool, second, 1)], timeout_s=30.0)
    _answers_match(pipeline, d, tool, [second], out)
    assert pipeline.engine.stats.snapshot()["hostFallbacks"] == before + 1
