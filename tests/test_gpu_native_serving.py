"""End-to-end native serving on GPU: C++ HTTP reactor -> GpuPipeline
(k_json2pb / k_pb2json) -> native h2 transport -> native backend."""

import http.client
import json
import threading

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native_gateway():
    from google.protobuf import descriptor_pb2

    from examples.protos import ALL_FDPS
    from ggrmcp_amd.backend.discovery import ServiceDiscoverer
    from ggrmcp_amd.backend.native_invoker import NativeWireClient, load_module
    from ggrmcp_amd.config import Config
    from ggrmcp_amd.engine.batch import GpuPipeline
    from ggrmcp_amd.server.native_http import NativeHTTPGateway
    from ggrmcp_amd.utils.synthetic import synthetic_fdp

    mod = load_module()
    srv = mod.Server("127.0.0.1:0")
    srv.add_route("/hello.HelloService/SayHello", "hello")
    srv.add_route("/bench.EchoService/Echo", "echo")
    srv.add_route("/bench.EchoService/StreamEcho", "stream_echo")
    bound = srv.start()

    cfg = Config.default()
    host, _, port = bound.rpartition(":")
    cfg.grpc.host, cfg.grpc.port = host, int(port)
    cfg.server.rate_limit_rps = 1_000_000
    cfg.server.rate_limit_burst = 1_000_000
    d = ServiceDiscoverer(cfg)
    fdset = descriptor_pb2.FileDescriptorSet()
    fdset.file.extend(ALL_FDPS + [synthetic_fdp()])
    d.load_descriptor_blob(fdset.SerializeToString())
    d.connections[0].connect(timeout_s=15)
    wire = NativeWireClient(bound, connections=2)
    pipeline = GpuPipeline(d, cfg, device=0, wire_clients=[wire])
    gw = NativeHTTPGateway(pipeline, d, cfg)
    port_http = gw.start()
    yield gw, port_http, pipeline, srv
    gw.stop()
    wire.close()
    d.close()
    srv.stop()


def _post(port, body, session=None):
    conn = http.client.HTTPConnection("127.0.0.1", port, timeout=15)
    headers = {"Content-Type": "application/json"}
    if session:
        headers["Mcp-Session-Id"] = session
    conn.request("POST", "/", body=body, headers=headers)
    r = conn.getresponse()
    data = r.read()
    sid = r.getheader("Mcp-Session-Id")
    conn.close()
    return r.status, json.loads(data), sid


def _gpu_ok(gw, pipeline):
    """GPU-completed requests across both serving paths: the Python
    batch_cb pipeline and the GIL-free native span (C++ counters)."""
    n = pipeline.engine.stats.gpu_ok
    if getattr(gw, "_span_engines", None):
        n += gw._fe.native_stats()["gpuOk"]
    return n


def test_serving_roundtrip_on_gpu(native_gateway):
    gw, port, pipeline = native_gateway[:3]
    before = _gpu_ok(gw, pipeline)
    body = json.dumps({"jsonrpc": "2.0", "id": 1, "method": "tools/call",
                       "params": {"name": "hello_helloservice_sayhello",
                                  "arguments": {"name": "serve"}}})
    status, resp, sid = _post(port, body)
    assert status == 200 and sid
    inner = json.loads(resp["result"]["content"][0]["text"])
    assert inner == {"message": "Hello, serve!"}
    assert _gpu_ok(gw, pipeline) > before  # GPU path, not fallback


def test_native_span_active_on_gpu(native_gateway):
    """The serving hot path must be the GIL-free C++ span (span_api.h) —
    not the Python batch_cb fallback (make the serving number
    the native number)."""
    gw, port, pipeline = native_gateway[:3]
    assert gw._span_engines, "native span must be enabled on the GPU path"
    st0 = gw._fe.native_stats()
    body = json.dumps({"jsonrpc": "2.0", "id": 11, "method": "tools/call",
                       "params": {"name": "hello_helloservice_sayhello",
                                  "arguments": {"name": "span"}}})
    status, resp, _ = _post(port, body)
    assert status == 200
    st1 = gw._fe.native_stats()
    assert st1["gpuOk"] > st0["gpuOk"]
    assert st1["requests"] > st0["requests"]
    assert st1["encodeMs"] > 0 and st1["decodeMs"] > 0


def test_native_span_grpc_error_envelope(native_gateway):
    """gRPC failure -> C++-assembled isError result (handler.go:252-259
    semantics) with the request id preserved from the kernel's id slot."""
    gw, port, pipeline = native_gateway[:3]
    body = json.dumps({"jsonrpc": "2.0", "id": "err-1", "method": "tools/call",
                       "params": {"name": "hello_helloservice_sayhello",
                                  "arguments": {"name": "error"}}})
    status, resp, _ = _post(port, body)
    assert status == 200
    assert resp["id"] == "err-1"
    assert resp["result"]["isError"] is True
    text = resp["result"]["content"][0]["text"]
    assert text.startswith("gRPC error INVALID_ARGUMENT")


def test_native_span_decode_fallback_single_invoke(native_gateway):
    """badutf8 response through the SERVING path: decode rejects, the
    fallback transcodes the delivered wire — zero duplicate invokes."""
    gw, port, pipeline = native_gateway[:3]
    body = json.dumps({"jsonrpc": "2.0", "id": 21, "method": "tools/call",
                       "params": {"name": "hello_helloservice_sayhello",
                                  "arguments": {"name": "badutf8"}}})
    srv = native_gateway[3]
    before = srv.request_count()
    status, resp, _ = _post(port, body)
    after = srv.request_count()
    assert status == 200
    assert resp["id"] == 21
    # both GPU and the protojson oracle reject invalid UTF-8 -> error
    # envelope, produced WITHOUT a second invoke
    assert "error" in resp
    assert after - before == 1, "fallback must not re-invoke" 


def _pipelined(port, bodies):
    """POST every body on one connection in a single send (HTTP/1.1
    pipelining), so the reactor parses them in one pass and hands them to
    the span executor together; returns the response bodies in order."""
    import socket

    req = b"".join(
        b"POST / HTTP/1.1\r\nHost: x\r\nContent-Type: application/json\r\n"
        b"Content-Length: %d\r\n\r\n%s" % (len(b), b) for b in bodies)
    out = []
    with socket.create_connection(("127.0.0.1", port), timeout=20) as s:
        s.sendall(req)
        buf = b""
        while len(out) < len(bodies):
            head, sep, rest = buf.partition(b"\r\n\r\n")
            clen = None
            if sep:
                for line in head.split(b"\r\n")[1:]:
                    k, _, v = line.partition(b":")
                    if k.strip().lower() == b"content-length":
                        clen = int(v)
            if clen is not None and len(rest) >= clen:
                assert head.startswith(b"HTTP/1.1 200"), head
                out.append(rest[:clen])
                buf = rest[clen:]
                continue
            chunk = s.recv(1 << 20)
            assert chunk, "connection closed early"
            buf += chunk
    return out


def test_both_span_paths_answer_alike(native_gateway):
    """One batch through Engine.process_span (GpuPipeline.process_batch with
    wire clients) and through Engine.run_span (the native frontend), same
    backend: every slot's response is the same JSON.  The two spans share
    their host phases and kernel launchers but keep their own error policy
    and envelope writers (C++ in run_span, Python for process_span's error
    slots), so each slot kind is compared.  Batch sizes: 1; WPB + 1 = 5 (a
    partial block); and all kinds next to a 64 KB echo, whose response is
    over the workgroup-decode threshold, so both decode kernels run in one
    span."""
    import random

    from ggrmcp_amd.utils.synthetic import wide_payload

    gw, port, pipeline = native_gateway[:3]

    def call(tool, args, **env):
        d = {"jsonrpc": "2.0", "id": 1, "method": "tools/call",
             "params": {"name": tool, "arguments": args}}
        d.update(env)
        return d

    hello = "hello_helloservice_sayhello"
    ok_1k = call(hello, {"name": "n" * 900}, id=7)
    assert 900 < len(json.dumps(ok_1k)) < 1100
    bad_arg = call(hello, {"nope": 1}, id=8)
    bad_tool = call("no_such_tool", {}, id=9)
    not_call = {"jsonrpc": "2.0", "id": 10, "method": "tools/list"}
    no_id = call(hello, {"name": "anon"})
    del no_id["id"]
    quoted_id = call(hello, {"name": "q"}, id='a"b')
    stream = call("bench_echoservice_streamecho",
                  {"f01String": "s", "f02Int32": 3}, id=11)
    grpc_err = call(hello, {"name": "error"}, id="err-2")
    big = call("bench_echoservice_echo",
               wide_payload(random.Random(7), target_bytes=64 * 1024), id=12)

    batches = [
        [ok_1k],
        [ok_1k, bad_arg, bad_tool, not_call, no_id],
        [big, ok_1k, bad_arg, bad_tool, not_call, no_id, quoted_id, stream,
         grpc_err],
    ]
    for batch in batches:
        bodies = [json.dumps(b).encode() for b in batch]
        st0 = gw._fe.native_stats()
        via_run_span = _pipelined(port, bodies)
        st1 = gw._fe.native_stats()
        spans = st1["batches"] - st0["batches"]
        print(len(bodies), "slots in", spans, "run_span call(s)")
        assert st1["requests"] - st0["requests"] == len(bodies)
        if sum(map(len, bodies)) < 16384:
            # one TCP segment on loopback: parsed and dispatched together
            assert spans == 1
        via_process_span = pipeline.process_batch(bodies, timeout_s=15.0)
        assert len(via_process_span) == len(via_run_span) == len(bodies)
        for req, a, b in zip(batch, via_process_span, via_run_span):
            assert json.loads(a) == json.loads(b), req.get("id")
    # the slots are what they are meant to be
    got = [json.loads(b) for b in via_run_span]
    assert got[0]["result"]["isError"] is False and got[0]["id"] == 12
    assert got[2]["error"]["code"] == -32602
    assert got[3]["error"]["code"] == -32601
    assert "tools" in got[4]["result"]
    assert got[5]["id"] is None and got[5]["result"]["isError"] is False
    assert got[6]["id"] == 'a"b'
    assert len(got[7]["result"]["content"]) == 3
    assert got[8]["result"]["content"][0]["text"].startswith(
        "gRPC error INVALID_ARGUMENT")


def test_serving_concurrent_sessions(native_gateway):
    gw, port, pipeline = native_gateway[:3]
    errs = []

    def worker(t):
        try:
            conn = http.client.HTTPConnection("127.0.0.1", port, timeout=15)
            for i in range(10):
                body = json.dumps({"jsonrpc": "2.0", "id": f"{t}-{i}",
                                   "method": "tools/call",
                                   "params": {"name": "hello_helloservice_sayhello",
                                              "arguments": {"name": f"u{t}x{i}"}}})
                conn.request("POST", "/", body=body,
                             headers={"Content-Type": "application/json"})
                r = conn.getresponse()
                resp = json.loads(r.read())
                assert resp["id"] == f"{t}-{i}"
                inner = json.loads(resp["result"]["content"][0]["text"])
                assert inner == {"message": f"Hello, u{t}x{i}!"}
            conn.close()
        except Exception as e:  # pragma: no cover
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(24)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


def test_serving_tools_list_and_errors(native_gateway):
    gw, port, pipeline = native_gateway[:3]
    status, resp, _ = _post(port, json.dumps(
        {"jsonrpc": "2.0", "id": 5, "method": "tools/list"}))
    assert status == 200
    names = [t["name"] for t in resp["result"]["tools"]]
    assert "hello_helloservice_sayhello" in names
    status, resp, _ = _post(port, json.dumps(
        {"jsonrpc": "2.0", "id": 6, "method": "tools/call",
         "params": {"name": "no_such_tool", "arguments": {}}}))
    assert resp["error"]["code"] == -32601
    status, resp, _ = _post(port, b"{broken")
    assert resp["error"]["code"] == -32700


def test_serving_soak_mixed(native_gateway):
    """Soak: concurrent sessions mixing unary, streaming, errors and
    malformed bodies through the reactor + native span; every response must
    match its request id and shape (order/captivity races would mispair)."""
    import random

    gw, port, pipeline = native_gateway[:3]
    errs = []

    def worker(t):
        rng = random.Random(t)
        try:
            conn = http.client.HTTPConnection("127.0.0.1", port, timeout=20)
            for i in range(25):
                kind = rng.randrange(5)
                rid = f"{t}-{i}"
                if kind == 0:
                    body = json.dumps({"jsonrpc": "2.0", "id": rid,
                                       "method": "tools/call",
                                       "params": {"name": "bench_echoservice_streamecho",
                                                  "arguments": {"f01String": rid,
                                                                "f02Int32": 3}}})
                elif kind == 1:
                    body = json.dumps({"jsonrpc": "2.0", "id": rid,
                                       "method": "tools/call",
                                       "params": {"name": "missing_tool",
                                                  "arguments": {}}})
                elif kind == 2:
                    body = json.dumps({"jsonrpc": "2.0", "id": rid,
                                       "method": "tools/list"})
                else:
                    body = json.dumps({"jsonrpc": "2.0", "id": rid,
                                       "method": "tools/call",
                                       "params": {"name": "hello_helloservice_sayhello",
                                                  "arguments": {"name": rid}}})
                conn.request("POST", "/", body=body,
                             headers={"Content-Type": "application/json"})
                r = conn.getresponse()
                resp = json.loads(r.read())
                assert resp["id"] == rid, (rid, resp)
                if kind == 0:
                    assert len(resp["result"]["content"]) == 3
                    inner = json.loads(resp["result"]["content"][1]["text"])
                    assert inner["f01String"] == rid
                elif kind == 1:
                    assert resp["error"]["code"] == -32601
                elif kind == 2:
                    assert "tools" in resp["result"]
                else:
                    inner = json.loads(resp["result"]["content"][0]["text"])
                    assert inner == {"message": f"Hello, {rid}!"}
            conn.close()
        except Exception as e:  # pragma: no cover
            errs.append((t, repr(e)))

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(32)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs[:3]


def test_serving_large_payloads_wg_kernels(native_gateway):
    """64 KB tool calls through the SERVING path: the workgroup-cooperative
    encode/decode kernels run inside the GIL-free span executor and the
    responses stay protojson-exact."""
    import random

    from ggrmcp_amd.engine.cpu_ref import CpuTranscoder
    from ggrmcp_amd.utils.synthetic import wide_payload

    gw, port, pipeline = native_gateway[:3]
    rng = random.Random(55)
    cpu = CpuTranscoder()
    d = gw.discoverer
    mi = d.tools["bench_echoservice_echo"]
    for i in range(4):
        args = wide_payload(rng, target_bytes=64 * 1024)
        body = json.dumps({"jsonrpc": "2.0", "id": 100 + i,
                           "method": "tools/call",
                           "params": {"name": "bench_echoservice_echo",
                                      "arguments": args}})
        status, resp, _ = _post(port, body)
        assert status == 200
        assert resp["id"] == 100 + i
        assert resp["result"]["isError"] is False, str(resp)[:300]
        inner = json.loads(resp["result"]["content"][0]["text"])
        wire = cpu.json_to_pb(mi.input_descriptor, json.dumps(args))
        oracle = json.loads(cpu.pb_to_json(mi.output_descriptor, wire))
        assert inner == oracle
