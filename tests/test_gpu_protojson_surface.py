"""protojson surface on gfx950: the corpus of tests/protojson_corpus.py
(same cases, same comparison rules as test_protojson_surface.py) through
the real 64-lane kernels.  One launch per list; a failing test lists every
failing case id."""

import pytest

import protojson_corpus as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from ggrmcp_amd.engine.batch import GpuEngine

    return pc.make_env(lambda infos: GpuEngine(infos, device=0))


@pytest.fixture(scope="module")
def wires(env):
    return pc.accept_wires(env)


def _report(res):
    bad = {k: v for k, v in res.items() if v}
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())


def test_gpu_accept_encode(env):
    _report(pc.run_encode(env, pc.ACCEPT))


def test_gpu_reject_encode(env):
    _report(pc.run_encode(env, pc.REJECT))


def test_gpu_python_lax_spellings_rejected(env):
    cases = pc.PY_LAX + pc.GO_STRICT
    enc, _ = env.engine.encode_batch(
        [c.data.encode() for c in cases], mode=1,
        msg_indices=[env.sink_idx] * len(cases), enforce=False)
    assert all(int(r["status"]) != 0 for r in enc), [int(r["status"]) for r in enc]


def test_gpu_accept_decode(env, wires):
    _report(pc.run_decode(env, pc.ACCEPT, wires, mode=1))


def test_gpu_accept_decode_envelope(env, wires):
    _report(pc.run_decode(env, pc.ACCEPT, wires, mode=0))


def test_gpu_wires_decode(env):
    _report(pc.run_decode(env, pc.WIRES, [c.data for c in pc.WIRES], mode=1))
