"""protojson surface + lane-window logic on the CPU (single-lane) build.

The corpus (tests/protojson_corpus.py) covers what the four production-
shaped schemas never reach: packed repeated scalars, every map key type,
the well-known types, long bytes and hand-assembled wire no well-behaved
serializer emits.  Each list runs as ONE kernel batch; the per-case tests
only report.  The @gpu twin (test_gpu_protojson_surface.py) runs the same
cases through the gfx950 build.
"""

import pytest

import protojson_corpus as pc
from ggrmcp_amd.engine.hostsim import HostSimEngine


@pytest.fixture(scope="module")
def env():
    return pc.make_env(HostSimEngine)


@pytest.fixture(scope="module")
def results(env):
    """Every batch of the corpus, run once: name -> {case id -> failure}."""
    aw = pc.accept_wires(env)
    return {
        "accept-encode": pc.run_encode(env, pc.ACCEPT),
        "reject-encode": pc.run_encode(env, pc.REJECT),
        "pylax-encode": pc.run_encode(env, pc.PY_LAX),
        "accept-decode": pc.run_decode(env, pc.ACCEPT, aw, mode=1),
        "accept-envelope": pc.run_decode(env, pc.ACCEPT, aw, mode=0),
        "wires-decode": pc.run_decode(env, pc.WIRES, [c.data for c in pc.WIRES],
                                      mode=1),
    }


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("cid", _ids(pc.ACCEPT))
def test_accept_encode(results, cid):
    assert results["accept-encode"][cid] is None, results["accept-encode"][cid]


@pytest.mark.parametrize("cid", _ids(pc.ACCEPT))
def test_accept_decode(results, cid):
    assert results["accept-decode"][cid] is None, results["accept-decode"][cid]


@pytest.mark.parametrize("cid", _ids(pc.ACCEPT))
def test_accept_decode_envelope(results, cid):
    assert results["accept-envelope"][cid] is None, results["accept-envelope"][cid]


@pytest.mark.parametrize("cid", _ids(pc.REJECT))
def test_reject_encode(env, results, cid):
    case = next(c for c in pc.REJECT if c.id == cid)
    assert pc.oracle_parse(env.sink_cls, case.data) is None, \
        "corpus error: the oracle accepts a REJECT payload"
    assert results["reject-encode"][cid] is None, results["reject-encode"][cid]


@pytest.mark.parametrize("case", pc.PY_LAX, ids=_ids(pc.PY_LAX))
def test_python_lax_spellings_rejected(env, case):
    """json_format accepts these; Go protojson does not (rules cited at
    PY_LAX).  Only the kernel's refusal is asserted."""
    enc, _ = env.engine.encode_batch([case.data.encode()], mode=1,
                                     msg_indices=[env.sink_idx], enforce=False)
    assert int(enc[0]["status"]) != 0


@pytest.mark.parametrize("cid", _ids(pc.WIRES))
def test_wires_decode(results, cid):
    assert results["wires-decode"][cid] is None, results["wires-decode"][cid]


@pytest.mark.parametrize("case", pc.GO_STRICT, ids=_ids(pc.GO_STRICT))
def test_go_strict_spellings_rejected(env, case):
    """Timestamp offsets and FieldMask paths Go refuses (rules at GO_STRICT)."""
    enc, _ = env.engine.encode_batch([case.data.encode()], mode=1,
                                     msg_indices=[env.sink_idx], enforce=False)
    assert int(enc[0]["status"]) != 0


def test_wires_oracle_verdicts_pinned(env):
    """The oracle refuses exactly the WIRES ids the corpus says it refuses."""
    refused = {c.id for c in pc.WIRES
               if pc.oracle_print(env.sink_cls, c.data) is None}
    assert refused == pc.WIRES_ORACLE_REJECTS, \
        sorted(refused ^ pc.WIRES_ORACLE_REJECTS)


def test_accept_oracle_verdicts(env):
    """Every ACCEPT payload is accepted by the oracle (PY_LAX/GO_STRICT too:
    they are only worth listing while Python still takes them)."""
    for c in pc.ACCEPT + pc.PY_LAX + pc.GO_STRICT:
        assert pc.oracle_parse(env.sink_cls, c.data) is not None, c.id


def test_corpus_shape():
    """The corpus' own budget: unique ids, HOST tags on at most one
    ACCEPT+WIRES case in eight, PY_LAX no larger than the three documented
    spellings and their direct variants."""
    for cases in (pc.ACCEPT, pc.REJECT, pc.WIRES, pc.PY_LAX, pc.GO_STRICT):
        assert len({c.id for c in cases}) == len(cases)
    tagged = [c for c in pc.ACCEPT + pc.WIRES if c.host]
    assert len(tagged) * pc.HOST_CAP <= len(pc.ACCEPT) + len(pc.WIRES)
    assert all(c.host is None for c in pc.REJECT + pc.PY_LAX)
    assert len(pc.PY_LAX) <= 8


def test_host_tags_cite_written_rules():
    """Every HOST tag quotes a rule that docs/KERNELS.md writes down."""
    from pathlib import Path

    doc = (Path(__file__).resolve().parent.parent / "docs" / "KERNELS.md").read_text()
    doc = " ".join(doc.split())
    for c in pc.ACCEPT + pc.WIRES:
        if c.host:
            assert c.host in doc, f"{c.id}: rule not in docs/KERNELS.md: {c.host}"


# ---- lane-window generators on the serial build --------------------------------
# WAVE=1 turns every window into a byte loop, so these pin the serial logic
# (and the generators themselves); test_gpu_lane_windows.py is the judge of
# the 64-lane forms.

def test_string_sweep(env):
    assert pc.check_string_sweep(env) is None


def test_utf8_defects_at_window_edges(env):
    assert pc.check_utf8(env) is None


def test_whitespace_runs(env):
    assert pc.check_whitespace(env) is None


def test_base64_lengths(env):
    assert pc.check_base64(env) is None


@pytest.mark.parametrize("n", pc.COMPACTION_SIZES)
def test_decode_batch_offsets(env, n):
    assert pc.check_compaction(env, n) is None
