"""Top-level packed runs split across the waves of ``k_pb2json_wg`` on gfx950: item
table, status, pad and bytes against the CPU build's for the cases of
``test_wg_packed_chunks.py``, text built in Python, batches through ``k_pack_out``."""

import json

import pytest

import packed_chunk_cases as cc
import packed_runs_corpus as pr
import protojson_corpus as pc
from test_gpu_packed_fixed_runs import _cpu, _gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def holders():
    return cc.make_holders(_gpu), cc.make_holders(_cpu)


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c[0])
def test_packed_run(holders, case):
    _, schema, wire, mode, status, text, items, ends = case
    gpu, cpu = holders[0][schema], holders[1][schema]
    table = gpu[0].wg_scan_probe(wire, gpu[2], mode)
    assert table == cpu[0].wg_scan_probe(wire, cpu[2], mode)
    assert [k for _, _, k in table] == items if items else len(table) >= 2
    got = pr.run_holder(gpu, wire, mode)
    assert got[:2] == (status, 1) and got == pr.run_holder(cpu, wire, mode)
    if status == 0:
        assert json.loads(got[2])["result"]["content"][0]["text"] == text


@pytest.mark.parametrize("n", [1, 17])
def test_batches_through_the_pack_kernel(holders, n):
    """Split, unsplit, classic-pass and short slots behind a filler of two lengths."""
    envs = [pc.Env(h[0], None, None, h[1], h[2], None, None, h[3], None, None)
            for h in (holders[0]["c"], holders[1]["c"])]
    wires = [cc.BATCH[i % len(cc.BATCH)][0] for i in range(n)]
    for filler in (1, 2):
        got = pr.run_batch(envs[0], wires, cc.UNPOP, filler)
        assert got == pr.run_batch(envs[1], wires, cc.UNPOP, filler)
        assert [g[:2] for g in got] == [cc.BATCH[i % len(cc.BATCH)][1] for i in range(n)]
