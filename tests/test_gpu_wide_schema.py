"""Wide schemas on gfx950: the lists of tests/wide_schema_corpus.py through
the real 64-lane kernels, one launch per list (the CPU twin is
test_wide_schema_surface.py).  Besides the oracle's verdict, every device
status and byte string must equal what the CPU build gives for the same
batch.  Encode also runs with GGRMCP_WG_ENC_MIN=1 (k_json2pb_wg), decode with
GGRMCP_WG_DEC_MIN=1 (k_pb2json_wg)."""

import os
from contextlib import contextmanager

import pytest

import wide_schema_corpus as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from ggrmcp_amd.engine.batch import GpuEngine

    return wc.make_env(lambda infos: GpuEngine(infos, device=0))


@pytest.fixture(scope="module")
def cpu():
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return wc.make_env(HostSimEngine)


@contextmanager
def _setenv(name, value):
    os.environ[name] = value
    try:
        yield
    finally:
        os.environ.pop(name, None)


def _report(res):
    bad = {k: v for k, v in res.items() if v}
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())


def _same_encode(cases, dev, ref):
    (enc_d, pbs_d), (enc_r, pbs_r) = dev, ref
    for c, d, r, pd, pr in zip(cases, enc_d, enc_r, pbs_d, pbs_r):
        assert int(d["status"]) == int(r["status"]), (
            c.id, int(d["status"]), int(r["status"]))
        assert (None if pd is None else bytes(pd)) == \
            (None if pr is None else bytes(pr)), c.id


@pytest.mark.parametrize("cases", [wc.ACCEPT, wc.REJECT, wc.GO_STRICT],
                         ids=["accept", "reject", "go-strict"])
@pytest.mark.parametrize("encode", [wc.encode_direct, wc.encode_envelope],
                         ids=["bare", "envelope"])
def test_gpu_encode(env, cpu, cases, encode):
    dev = encode(env, cases)
    if cases is wc.GO_STRICT:
        assert all(int(r["status"]) != 0 for r in dev[0])
    else:
        _report(wc.pc.encode_verdicts(
            cases, [env.cls[c.msg] for c in cases], *dev))
    _same_encode(cases, dev, encode(cpu, cases))


@pytest.mark.parametrize("cases", [wc.ACCEPT, wc.REJECT, wc.GO_STRICT],
                         ids=["accept", "reject", "go-strict"])
def test_gpu_encode_workgroup(env, cpu, cases):
    """The same envelopes through k_json2pb_wg (serial scanner: the
    arguments are far below 8 KB)."""
    with _setenv("GGRMCP_WG_ENC_MIN", "1"):
        dev = wc.encode_envelope(env, cases)
    if cases is wc.GO_STRICT:
        assert all(int(r["status"]) != 0 for r in dev[0])
    else:
        _report(wc.pc.encode_verdicts(
            cases, [env.cls[c.msg] for c in cases], *dev))
    _same_encode(cases, dev, wc.encode_envelope(cpu, cases))


@pytest.mark.parametrize("wg", [False, True], ids=["classic", "workgroup"])
@pytest.mark.parametrize("flags", [0, wc.DM_UNPOPULATED], ids=["plain", "unpop"])
def test_gpu_wires_decode(env, cpu, flags, wg):
    cases = wc.wires(env, flags)
    with _setenv("GGRMCP_WG_DEC_MIN", "1" if wg else "1000000000"):
        res, raw = wc.run_decode(env, cases, flags)
        ref_res, ref_raw = wc.run_decode(cpu, cases, flags, wg=wg)
    _report(res)
    _report(ref_res)
    for c, d, r in zip(cases, raw, ref_raw):
        assert d == r, (c.id, d, r)
