"""Native serving span over the gathered h2 transport, on GPU: many
concurrent keep-alive sessions through the C++ reactor -> span executor ->
native h2 client -> native backend.  Checks pairing (every response carries
its own request's name), exactly-once invocation, and that the span's batches
really leave in gathered sends (wire-client counters)."""

import http.client
import json
import socket

import pytest

pytestmark = pytest.mark.gpu

SESSIONS = 130
POSTS = 5
# (session, post) slots that carry a special name
ERROR_SLOTS = {(7, 1), (101, 3)}
BADUTF8_SLOT = (64, 2)


@pytest.fixture(scope="module")
def span_gateway():
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


def _name(t, i):
    if (t, i) in ERROR_SLOTS:
        return "error"
    if (t, i) == BADUTF8_SLOT:
        return "badutf8"
    return f"s{t}p{i}"


def test_concurrent_sessions_over_gathered_transport(span_gateway):
    gw, port, pipeline, srv = span_gateway
    assert gw._span_engines, "native span must be the serving path"
    wire = pipeline.wire_clients[0]

    # The sessions must really have their requests in flight together, or the
    # span executor sees batches of one or two calls and there is nothing to
    # gather (130 http.client threads serialise on the interpreter lock and
    # reach about 1.6 calls per batch).  So one driver owns all 130
    # keep-alive sockets: it writes one prepared request on each, then reads
    # the 130 responses, five times over.
    socks = [socket.create_connection(("127.0.0.1", port), timeout=20)
             for _ in range(SESSIONS)]
    for s in socks:
        s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)

    def request(t, i):
        body = json.dumps({"jsonrpc": "2.0", "id": f"{t}-{i}",
                           "method": "tools/call",
                           "params": {"name": "hello_helloservice_sayhello",
                                      "arguments": {"name": _name(t, i)}}}).encode()
        return (b"POST / HTTP/1.1\r\nHost: 127.0.0.1\r\n"
                b"Content-Type: application/json\r\n"
                b"Content-Length: %d\r\n\r\n" % len(body)) + body

    w0 = wire.stats()
    r0 = srv.request_count()
    try:
        for i in range(POSTS):
            wires = [request(t, i) for t in range(SESSIONS)]
            for s, w in zip(socks, wires):
                s.sendall(w)
            for t, s in enumerate(socks):
                r = http.client.HTTPResponse(s, method="POST")
                r.begin()
                resp = json.loads(r.read())
                assert not r.will_close  # the session stays open
                rid, name = f"{t}-{i}", _name(t, i)
                assert resp["id"] == rid, (rid, resp)
                if name == "error":
                    assert resp["result"]["isError"] is True
                    text = resp["result"]["content"][0]["text"]
                    assert text.startswith("gRPC error INVALID_ARGUMENT"), text
                elif name == "badutf8":
                    assert "error" in resp, resp
                else:
                    inner = json.loads(resp["result"]["content"][0]["text"])
                    assert inner == {"message": f"Hello, {name}!"}, (rid, inner)
    finally:
        for s in socks:
            s.close()
    w1 = wire.stats()
    r1 = srv.request_count()
    total = SESSIONS * POSTS
    calls = w1["calls"] - w0["calls"]
    sends = w1["send_calls"] - w0["send_calls"]
    batches = w1["batches"] - w0["batches"]
    print(f"{calls} calls in {batches} batches, {sends} client send() calls "
          f"({sends / max(calls, 1):.3f} per call)")
    assert r1 - r0 == total  # every request invoked exactly once
    assert calls == total
    assert sends <= calls / 4
