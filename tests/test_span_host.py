"""The native spans' pure host pieces (ops/csrc/span_host.h) on the CPU tier.

Engine.process_span and Engine.run_span share one gRPC reply parser and one
pair of error-envelope builders; _hostsim binds them so the frame rules and
the envelope texts are pinned without a GPU.  The envelopes are compared
with what GpuPipeline._host_slot assembles for the same slot, since a
client must not be able to tell which path answered it.
"""

import json
import struct
from types import SimpleNamespace

import pytest

from ggrmcp_amd.backend.native_invoker import _CODE_NAMES, NativeRpcError
from ggrmcp_amd.engine import batch
from ggrmcp_amd.engine.hostsim import load_module

hs = load_module()

TRUNCATED = "truncated gRPC frame"
COMPRESSED = "compressed gRPC response frame not supported"
STATUSLESS = "stream closed without grpc-status"


def frame(flag: int, declared: int, payload: bytes = b"") -> bytes:
    return bytes([flag]) + struct.pack(">I", declared) + payload


# ---- frame rules -----------------------------------------------------------

@pytest.mark.parametrize(
    "status, data, msg, want",
    [
        (0, b"", "", (0, 0, 0, None)),
        (0, frame(0, 0), "", (0, 5, 0, None)),
        (0, frame(0, 3, b"abc"), "", (0, 5, 3, None)),
        (0, frame(0, 3, b"abc") + b"tail", "", (0, 5, 3, None)),
        (0, b"\0", "", (13, 0, 0, TRUNCATED)),
        (0, b"\0\0", "", (13, 0, 0, TRUNCATED)),
        (0, b"\0\0\0", "", (13, 0, 0, TRUNCATED)),
        (0, b"\0\0\0\0", "", (13, 0, 0, TRUNCATED)),
        (0, frame(0, 4, b"abc"), "", (13, 0, 0, TRUNCATED)),
        # the 32-bit edge: 5 + 0xFFFFFFFF must not wrap to 4
        (0, frame(0, 0xFFFFFFFF), "", (13, 0, 0, TRUNCATED)),
        (0, frame(1, 0), "", (13, 0, 0, COMPRESSED)),
        # Compressed AND short.  With a whole 5-byte prefix the flag is read
        # before the length test, and the verdict ladder asks `status == 0 &&
        # compressed` before `status == 0 && truncated` (engine.cpp of the
        # parent commit, process_span: the `else if (status == 0 &&
        # compressed)` branch precedes the truncated one), so the verdict is
        # "compressed".  Under 5 bytes the flag is never read: "truncated".
        (0, frame(1, 4, b"abc"), "", (13, 0, 0, COMPRESSED)),
        (0, b"\1\0\0", "", (13, 0, 0, TRUNCATED)),
        (-1, b"", "", (2, 0, 0, STATUSLESS)),
        (-1, frame(0, 3, b"abc"), "", (2, 0, 0, STATUSLESS)),
        (-1, b"", "peer reset", (2, 0, 0, "peer reset")),
        # a non-zero status wins over a good frame
        (5, frame(0, 3, b"abc"), "no such thing", (5, 0, 0, "no such thing")),
        (5, frame(1, 9, b"abc"), "no such thing", (5, 0, 0, "no such thing")),
    ],
)
def test_grpc_reply(status, data, msg, want):
    assert hs.grpc_reply(status, data, msg) == want


# ---- envelopes -------------------------------------------------------------

# raw JSON-RPC id tokens as the encode kernel captures them (None: no id)
IDS = [b"1", b'"a\\"b"', None, b'"' + b"x" * 62 + b'"']  # the last: 64 bytes
DETAILS = ['"', "\\", "\n", "\r", "\t", "\x01", "\x1f", "héllo ✓ \U0001f600",
           'all: " \\ \n \r \t \x01 \x1f é', ""]


def host_slot(id_token, status, rpc_err):
    """What the Python host path answers for the same slot."""
    pipe = object.__new__(batch.GpuPipeline)
    pipe.non_toolcall_handler = None
    engine = SimpleNamespace(stats=batch.EngineStats())
    body = b'{"jsonrpc":"2.0","method":"tools/call"'
    if id_token is not None:
        body += b',"id":' + id_token
    body += b"}"
    out = pipe._host_slot(engine, body, {"status": status, "flags": 0}, None,
                          None, rpc_err, None, None)
    assert engine.stats.errors == 1
    return json.loads(out)


@pytest.mark.parametrize("id_token", IDS)
@pytest.mark.parametrize("detail", DETAILS)
def test_grpc_error_envelope_matches_host_slot(id_token, detail):
    got = hs.grpc_error_envelope(id_token, 14, detail)
    assert json.loads(got) == host_slot(id_token, batch.E_OK,
                                        NativeRpcError(14, detail))


@pytest.mark.parametrize("id_token", IDS)
@pytest.mark.parametrize("status", sorted(batch._STATUS_TO_RPC) + [99])
def test_rpc_error_envelope_matches_host_slot(id_token, status):
    code, msg = batch._STATUS_TO_RPC.get(status, (-32603, "internal error"))
    got = hs.rpc_error_envelope(id_token, code, msg)
    assert json.loads(got) == host_slot(id_token, status, None)


@pytest.mark.parametrize("detail", DETAILS)
def test_rpc_error_envelope_escapes_its_message(detail):
    got = json.loads(hs.rpc_error_envelope(b"7", -32603, detail))
    assert got == {"jsonrpc": "2.0", "id": 7,
                   "error": {"code": -32603, "message": detail}}


def test_status_to_rpc_matches_python_table():
    # E_NOT_TOOLCALL never reaches the C++ mapping (run_span hands those
    # slots to the Python MCP handler), so it is not in the C++ table
    for status, want in batch._STATUS_TO_RPC.items():
        if status != batch.E_NOT_TOOLCALL:
            assert hs.status_to_rpc(status) == want
    for status in (batch.E_OK, batch.E_NOT_TOOLCALL, 99, -1):
        assert hs.status_to_rpc(status) == (-32603, "internal error")


def test_grpc_status_names():
    def name(code):
        text = json.loads(hs.grpc_error_envelope(b"1", code, "d"))
        return text["result"]["content"][0]["text"]

    assert len(_CODE_NAMES) == 17
    for code in range(17):
        assert name(code) == f"gRPC error {_CODE_NAMES[code]}: d"
        assert str(NativeRpcError(code, "d")) == f"{_CODE_NAMES[code]}: d"
    assert name(17) == "gRPC error CODE_?: d"
    assert name(-1) == "gRPC error CODE_?: d"
