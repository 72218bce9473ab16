"""DM_REORDER on the CPU tier: the phases of ``k_pb_reorder`` (pb_reorder.h)
driven at WAVE=1 by ``reorder_host`` behind the CPU build's decode kernels,
over ``reorder_corpus.CASES``, judged by the protojson oracle."""

import pytest

import protojson_corpus as pc
import reorder_corpus as rc
import unpopulated_corpus as uc
import wg_flags_corpus as wc
from ggrmcp_amd.engine.hostsim import HostSimEngine

RO, MODES = rc.RO, rc.MODES


@pytest.fixture(scope="module")
def envs():
    return rc.make_envs(HostSimEngine)


@pytest.fixture(scope="module")
def wg_envs():
    return rc.make_envs(lambda infos: HostSimEngine(infos, wg=True))


@pytest.fixture(scope="module")
def answers(envs):
    return {m: rc.run(envs, list(rc.CASES), m) for m in MODES}


@pytest.mark.parametrize("cid", list(rc.CASES))
def test_case(envs, answers, cid):
    """Every kind and flag set (judge fails an "ok" case the oracle refuses);
    with the flag clear the slot is E_UNSUPPORTED."""
    for m in MODES:
        assert rc.judge(envs, cid, m, answers[m][cid]) is None, (cid, m)
    st, _, pad, _ = rc.run(envs, [cid], 1)[cid]
    assert st != 0 and pad == 0
    if rc.CASES[cid][2] != "refused":
        assert st == pc.E_UNSUPPORTED


def test_big_slot_refused_by_the_workgroup_kernel(wg_envs):
    """A >= 16 KB envelope slot k_pb2json_wg refuses is decoded by one wave."""
    for flags in (0, uc.DM_UNPOPULATED | uc.DM_STRUCTURED):
        got = rc.run(wg_envs, ["unknowns-big", "swap-top"], 0 | RO | flags)
        assert not [c for c in got if rc.judge(wg_envs, c, 0 | RO | flags, got[c])]
        assert wc.run(wg_envs.base, {"b": rc.CASES["unknowns-big"][:2]}, 0)["b"][2] in (1, 2)


@pytest.mark.parametrize("flags", wc.FLAG_SETS)
def test_in_order_wires_do_not_move(envs, flags):
    """Every in-order status-0 wire of wg_flags_corpus: same bytes and pad."""
    cases = wc.all_cases(envs.base)
    off, on = wc.run(envs.base, cases, flags), wc.run(envs.base, cases, flags | RO)
    same = [c for c in cases if off[c][0] == 0]
    assert len(same) > 100 and all(off[c][:3] == on[c][:3] for c in same)
