"""google.protobuf.Any on the CPU (single-lane) build of the kernels.

The corpus (tests/any_corpus.py) runs each list as ONE kernel batch through
HostSimEngine; the per-case tests only report.  The oracle is json_format
with the schema's own descriptor pool.  The @gpu twin (test_gpu_any.py) runs
the same cases through the gfx950 build.
"""

from pathlib import Path

import pytest

import any_corpus as ac
from ggrmcp_amd.engine.hostsim import HostSimEngine


@pytest.fixture(scope="module")
def env():
    return ac.make_env(HostSimEngine)


@pytest.fixture(scope="module")
def results(env):
    """Every batch of the corpus, run once: name -> {case id -> failure}."""
    aw = ac.accept_wires(env)
    wires = [c.data for c in ac.WIRES]
    return {
        "accept-encode": ac.run_encode(env, ac.ACCEPT),
        "reject-encode": ac.run_encode(env, ac.REJECT),
        "decides-encode": ac.run_encode(env, ac.ORACLE_DECIDES),
        "accept-decode": ac.run_decode(env, ac.ACCEPT, aw, mode=1),
        "accept-envelope": ac.run_decode(env, ac.ACCEPT, aw, mode=0),
        "wires-decode": ac.run_decode(env, ac.WIRES, wires, mode=1),
        "wires-envelope": ac.run_decode(env, ac.WIRES, wires, mode=0),
    }


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("cid", _ids(ac.ACCEPT))
def test_accept_encode(results, cid):
    assert results["accept-encode"][cid] is None, results["accept-encode"][cid]


@pytest.mark.parametrize("cid", _ids(ac.ACCEPT))
def test_accept_decode(results, cid):
    assert results["accept-decode"][cid] is None, results["accept-decode"][cid]


@pytest.mark.parametrize("cid", _ids(ac.ACCEPT))
def test_accept_decode_envelope(results, cid):
    assert results["accept-envelope"][cid] is None, results["accept-envelope"][cid]


@pytest.mark.parametrize("cid", _ids(ac.REJECT))
def test_reject_encode(env, results, cid):
    case = next(c for c in ac.REJECT if c.id == cid)
    assert ac.oracle_parse(env, case.data) is None, \
        "corpus error: the oracle accepts a REJECT payload"
    assert results["reject-encode"][cid] is None, results["reject-encode"][cid]


@pytest.mark.parametrize("cid", _ids(ac.ORACLE_DECIDES))
def test_oracle_decides_encode(results, cid):
    """WKT payloads without "value", Empty via "value": protojson
    implementations differ, so the oracle's verdict is taken as it comes."""
    assert results["decides-encode"][cid] is None, results["decides-encode"][cid]


@pytest.mark.parametrize("cid", _ids(ac.WIRES))
def test_wires_decode(results, cid):
    assert results["wires-decode"][cid] is None, results["wires-decode"][cid]


@pytest.mark.parametrize("cid", _ids(ac.WIRES))
def test_wires_decode_envelope(results, cid):
    assert results["wires-envelope"][cid] is None, results["wires-envelope"][cid]


def test_accept_oracle_verdicts(env):
    """Every ACCEPT payload is accepted by the oracle, and the device-handled
    ones are answered ON the device build (status 0), not merely allowed to."""
    for c in ac.ACCEPT:
        assert ac.oracle_parse(env, c.data) is not None, c.id
    plain = [c for c in ac.ACCEPT if not c.host]
    enc, _ = env.engine.encode_batch([c.data.encode() for c in plain], mode=1,
                                     msg_indices=[env.idx] * len(plain),
                                     enforce=False)
    assert [c.id for c, r in zip(plain, enc) if int(r["status"])] == []
    wires = [w for c, w in zip(ac.ACCEPT, ac.accept_wires(env)) if not c.host]
    dec, _ = env.engine.decode_batch(wires, [env.idx] * len(wires), mode=1)
    assert [c.id for c, r in zip(plain, dec) if int(r["status"])] == []


def test_wires_oracle_accepts_the_host_tagged(env):
    """A HOST tag on a wire only means something where the oracle accepts."""
    for c in ac.WIRES:
        if c.host:
            assert ac.oracle_print(env, c.data) is not None, c.id
    for cid in ("canonical", "empty-any", "url-only", "url-only-wkt",
                "wkt-value", "empty-value", "nonminimal-lengths",
                "in-ra-and-ma"):
        case = next(c for c in ac.WIRES if c.id == cid)
        assert ac.oracle_print(env, case.data) is not None, cid


def test_corpus_shape():
    """Unique ids; HOST tags on at most one ACCEPT+WIRES case in eight and on
    no REJECT case."""
    for cases in (ac.ACCEPT, ac.REJECT, ac.ORACLE_DECIDES, ac.WIRES):
        assert len({c.id for c in cases}) == len(cases)
    tagged = [c for c in ac.ACCEPT + ac.WIRES if c.host]
    assert len(tagged) * ac.HOST_CAP <= len(ac.ACCEPT) + len(ac.WIRES)
    assert all(c.host is None for c in ac.REJECT + ac.ORACLE_DECIDES)


def test_host_tags_cite_written_rules():
    """Every HOST tag quotes a rule that docs/KERNELS.md writes down."""
    doc = (Path(__file__).resolve().parent.parent / "docs" / "KERNELS.md").read_text()
    doc = " ".join(doc.split())
    for c in ac.ACCEPT + ac.WIRES:
        if c.host:
            assert c.host in doc, f"{c.id}: rule not in docs/KERNELS.md: {c.host}"


def test_stranger_is_not_loaded(env):
    """v/stranger.proto builds, but neither the pool nor the tables know it."""
    assert ac.stranger_fdp().message_type[0].name == "Stranger"
    with pytest.raises(KeyError):
        env.pool.FindMessageTypeByName("v.Stranger")
    assert "v.Stranger" not in env.engine.tables.msg_index


def test_top_level_any_goes_to_the_host(env):
    """A tool whose message is itself an Any leaves both kernels with
    E_UNSUPPORTED (docs/KERNELS.md host-escape rules)."""
    any_idx = env.engine.tables.msg_index["google.protobuf.Any"]
    enc, _ = env.engine.encode_batch(
        [ac._j(ac.LEAF).encode()], mode=1, msg_indices=[any_idx], enforce=False)
    assert int(enc[0]["status"]) == 6
    wire = ac.ld(1, b"t.Leaf")
    dec, _ = env.engine.decode_batch([wire], [any_idx], mode=1)
    assert int(dec[0]["status"]) == 6


def test_mixed_batch_slots_are_independent(env):
    """One launch with Any slots interleaved with plain t.Leaf slots and
    failing slots: a slot's status and bytes do not depend on its neighbours
    (same answers in reverse order and alone), and match the oracle."""
    anys = [c for c in ac.ACCEPT if not c.host][:24]
    bad = ac.REJECT[:8]
    slots = []      # (payload, msg index)
    for i, c in enumerate(anys):
        slots.append((c.data.encode(), env.idx))
        slots.append((b'{"id":%d,"tag":"leaf"}' % i, env.leaf_idx))
        if i < len(bad):
            slots.append((bad[i].data.encode(), env.idx))

    def run(order):
        enc, pbs = env.engine.encode_batch(
            [slots[k][0] for k in order], mode=1,
            msg_indices=[slots[k][1] for k in order], enforce=False)
        return {k: (int(r["status"]), pb) for k, r, pb in zip(order, enc, pbs)}

    fwd = run(list(range(len(slots))))
    rev = run(list(reversed(range(len(slots)))))
    assert fwd == rev
    for k in (0, 1, 2, len(slots) - 1):
        assert run([k])[k] == fwd[k]
    # the Any slots against the oracle, the failing ones non-zero
    k = 0
    for i, c in enumerate(anys):
        res = ac.encode_verdicts(env, [c], [{"status": fwd[k][0], "aux": 0}],
                                 [fwd[k][1]])
        assert res[c.id] is None, res[c.id]
        assert fwd[k + 1][0] == 0
        k += 2
        if i < len(bad):
            assert fwd[k][0] != 0, bad[i].id
            k += 1

    # and the same interleaving on decode
    aw = dict(zip([c.id for c in ac.ACCEPT], ac.accept_wires(env)))
    dslots = []
    for i, c in enumerate(anys):
        dslots.append((aw[c.id], env.idx))
        dslots.append((ac.tag(1, 0) + ac.vi(i + 1), env.leaf_idx))
        dslots.append((ac.WIRES[-1 - (i % 8)].data, env.idx))

    def drun(order):
        dec, outs = env.engine.decode_batch(
            [dslots[k][0] for k in order], [dslots[k][1] for k in order], mode=1)
        return {k: (int(r["status"]), o) for k, r, o in zip(order, dec, outs)}

    dfwd = drun(list(range(len(dslots))))
    assert dfwd == drun(list(reversed(range(len(dslots)))))
    for i, c in enumerate(anys):
        st, out = dfwd[3 * i]
        res = ac.decode_verdicts(env, [c], [aw[c.id]], [{"status": st}], [out],
                                 lambda o: o)
        assert res[c.id] is None, res[c.id]
        assert dfwd[3 * i + 1] == (0, b'{"id":%d}' % (i + 1))
