"""google.protobuf.Any on the host path: the CPU transcoder (the kernels'
fallback) and a tools/call through the MCP handler without a GPU engine.

The gateway's descriptors live in a private pool, so the host transcodes must
hand json_format that pool — protobuf's default pool does not know the
backend's types."""

import asyncio
import json

import pytest
from google.protobuf import descriptor_pb2, json_format

import any_corpus as ac
from ggrmcp_amd.engine.cpu_ref import CpuTranscoder

PROBE = '{"a":{"@type":"type.googleapis.com/t.Leaf","id":5,"tag":"x"},"after":"z"}'


def test_cpu_transcoder_round_trips_any():
    pool, _ = ac.make_infos()
    desc = pool.FindMessageTypeByName("t.Holder")
    cpu = CpuTranscoder()
    wire = cpu.json_to_pb(desc, PROBE)
    msg = cpu.pb_to_message(desc, wire)
    assert msg.a.type_url == "type.googleapis.com/t.Leaf"
    assert msg.a.value == b"\x08\x05\x12\x01x"
    assert msg.after == "z"
    assert json.loads(cpu.pb_to_json(desc, wire)) == json.loads(PROBE)


def test_cpu_transcoder_still_refuses_unloaded_types():
    pool, _ = ac.make_infos()
    desc = pool.FindMessageTypeByName("t.Holder")
    cpu = CpuTranscoder()
    with pytest.raises(json_format.ParseError):
        cpu.json_to_pb(desc, '{"a":{"@type":"v.Stranger","x":1}}')


@pytest.fixture(scope="module")
def gateway():
    from ggrmcp_amd.backend.discovery import ServiceDiscoverer
    from ggrmcp_amd.backend.native_invoker import load_module
    from ggrmcp_amd.config import Config
    from ggrmcp_amd.server.handler import MCPHandler

    srv = load_module().Server("127.0.0.1:0")
    srv.add_route("/t.AnyService/Echo", "echo")
    bound = srv.start()
    cfg = Config.default()
    host, _, port = bound.rpartition(":")
    cfg.grpc.host, cfg.grpc.port = host, int(port)
    d = ServiceDiscoverer(cfg)
    fdset = descriptor_pb2.FileDescriptorSet()
    fdset.file.extend([ac.other_fdp(), ac.anyh_fdp()])
    d.load_descriptor_blob(fdset.SerializeToString())
    d.connections[0].connect(timeout_s=15)
    # no engine: the handler transcodes on the CPU, as under --no-gpu
    handler = MCPHandler(d, config=cfg)
    yield handler, d
    d.close()
    srv.stop()


def test_tools_call_echoes_any_without_gpu(gateway):
    from ggrmcp_amd.server.middleware import Request

    handler, d = gateway
    tool = next(n for n in d.tools if n.endswith("echo"))
    args = json.loads(PROBE)
    args["ra"] = [{"@type": "t.Orphan", "n": "7"}, {}]
    req = Request(
        method="POST", path="/", headers={"content-type": "application/json"},
        body=json.dumps({"jsonrpc": "2.0", "id": 1, "method": "tools/call",
                         "params": {"name": tool, "arguments": args}}).encode())
    resp = asyncio.run(handler.handle(req))
    body = json.loads(resp.body)
    assert body["result"]["isError"] is False, body
    assert json.loads(body["result"]["content"][0]["text"]) == args
