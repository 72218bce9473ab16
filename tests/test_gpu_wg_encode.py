"""Workgroup-cooperative encode (k_json2pb_wg) differential tests.

Large requests route one-workgroup-per-request; member items and chunked
map/repeated runs must concatenate into wire BYTES identical to the
classic per-wave kernel (protobuf concatenation semantics), and the
end-to-end pipeline must stay protojson-exact.  GGRMCP_WG_ENC_MIN forces
both paths over identical payloads."""

import json
import os
import random

import pytest

pytestmark = pytest.mark.gpu

from test_gpu_wg_decode import _body, _first_diff, _shapes, env  # noqa: F401,E402
from ggrmcp_amd.engine.batch import SR_WG_CLASSIC, SR_WG_ITEMS  # noqa: E402


def test_wg_encode_matches_classic_bytes(env):  # noqa: F811
    """Classic vs cooperative ENCODE wire must be byte-identical."""
    pipeline, d = env
    bodies = [_body(a, i + 1) for i, a in enumerate(_shapes())]

    os.environ["GGRMCP_WG_ENC_MIN"] = "1000000000"
    enc_a, pbs_a = pipeline.engine.encode_batch(bodies, mode=0)
    os.environ["GGRMCP_WG_ENC_MIN"] = "4096"
    enc_b, pbs_b = pipeline.engine.encode_batch(bodies, mode=0)
    os.environ.pop("GGRMCP_WG_ENC_MIN", None)

    for i in range(len(bodies)):
        assert enc_a[i]["status"] == enc_b[i]["status"], i
        assert enc_a[i]["tool_idx"] == enc_b[i]["tool_idx"], i
        assert enc_a[i]["id_len"] == enc_b[i]["id_len"], i
        assert pbs_a[i] == pbs_b[i], (
            f"slot {i} wire diverged: {len(pbs_a[i] or b'')}B vs "
            f"{len(pbs_b[i] or b'')}B")


def test_wg_encode_end_to_end_oracle(env):  # noqa: F811
    """Forced-wg encode through the full pipeline stays protojson-exact."""
    pipeline, d = env
    shapes = _shapes()
    bodies = [_body(a, i + 1) for i, a in enumerate(shapes)]
    os.environ["GGRMCP_WG_ENC_MIN"] = "4096"
    try:
        out = pipeline.process_batch(bodies, timeout_s=30.0)
    finally:
        os.environ.pop("GGRMCP_WG_ENC_MIN", None)
    mi = d.tools["bench_echoservice_echo"]
    for i, (args, raw) in enumerate(zip(shapes, out)):
        resp = json.loads(raw)
        assert resp["result"]["isError"] is False, resp
        inner = json.loads(resp["result"]["content"][0]["text"])
        wire = pipeline.cpu.json_to_pb(mi.input_descriptor, json.dumps(args))
        oracle = json.loads(pipeline.cpu.pb_to_json(mi.output_descriptor, wire))
        assert inner == oracle, f"slot {i}: {_first_diff(inner, oracle)}"


def test_wg_encode_fuzz_vs_classic(env):  # noqa: F811
    from ggrmcp_amd.utils.synthetic import wide_payload

    pipeline, d = env
    rng = random.Random(123)
    bodies = [
        _body(wide_payload(rng, target_bytes=rng.choice(
            [9000, 17000, 30000, 64000])), i)
        for i in range(48)
    ]
    os.environ["GGRMCP_WG_ENC_MIN"] = "1000000000"
    enc_a, pbs_a = pipeline.engine.encode_batch(bodies, mode=0)
    os.environ["GGRMCP_WG_ENC_MIN"] = "2048"
    enc_b, pbs_b = pipeline.engine.encode_batch(bodies, mode=0)
    os.environ.pop("GGRMCP_WG_ENC_MIN", None)
    for i in range(len(bodies)):
        assert enc_a[i]["status"] == enc_b[i]["status"], i
        assert pbs_a[i] == pbs_b[i], f"slot {i} wire diverged"


def test_wg_encode_error_paths(env):  # noqa: F811
    """Errors must match the classic kernel exactly (the wg path falls back
    to an in-block classic pass for anomalies)."""
    pipeline, d = env
    big_pad = {"attrs": {f"p{j}": "x" * 900 for j in range(24)}}
    cases = [
        # unknown field in a big payload
        {"nosuchfield": 1, **big_pad},
        # duplicate member (json.dumps would dedupe a dict; craft manually)
        None,
        # oneof-free dup via repeated key string below
    ]
    bodies = [_body(cases[0], 1)]
    pad = ",".join(f'"z{j}": "' + "y" * 900 + '"' for j in range(4))
    dup = ('{"jsonrpc":"2.0","id":2,"method":"tools/call","params":'
           '{"name":"bench_echoservice_echo","arguments":{'
           '"f02Int32":1,"f02Int32":2,"attrs":{' + pad + "}}}}")
    bodies.append(dup.encode())
    os.environ["GGRMCP_WG_ENC_MIN"] = "1000000000"
    enc_a, _ = pipeline.engine.encode_batch(bodies, mode=0)
    os.environ["GGRMCP_WG_ENC_MIN"] = "1024"
    enc_b, _ = pipeline.engine.encode_batch(bodies, mode=0)
    os.environ.pop("GGRMCP_WG_ENC_MIN", None)
    for i in range(len(bodies)):
        assert enc_a[i]["status"] == enc_b[i]["status"], (
            i, enc_a[i]["status"], enc_b[i]["status"])
        assert enc_a[i]["err_pos"] == enc_b[i]["err_pos"], i
        assert enc_a[i]["aux"] == enc_b[i]["aux"], i
        # both are scanner anomalies: the in-block classic pass answered, and
        # the classic kernel tags no path
        assert enc_b[i]["status"] != 0
        assert enc_b[i]["flags"] & (SR_WG_ITEMS | SR_WG_CLASSIC) == SR_WG_CLASSIC, i
        assert enc_a[i]["flags"] & (SR_WG_ITEMS | SR_WG_CLASSIC) == 0, i
