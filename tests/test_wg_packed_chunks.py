"""Top-level packed runs split across the items of ``k_pb2json_wg``, CPU build: the
item table (``wg_scan_probe``), the joined text against text built in Python and
``json_format``, status and bytes against ``k_pb2json``."""

import json

import pytest

import packed_chunk_cases as cc
import packed_runs_corpus as pr
import protojson_corpus as pc


@pytest.fixture(scope="module")
def holders():
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return cc.make_holders(lambda infos: HostSimEngine(infos, wg=True))


@pytest.mark.parametrize("case", cc.CASES + cc.CPU_ONLY, ids=lambda c: c[0])
def test_packed_run(holders, case):
    _, schema, wire, mode, status, text, items, ends = case
    h = holders[schema]
    table = h[0].wg_scan_probe(wire, h[2], mode)
    kinds = [k for _, _, k in table]
    assert len(kinds) <= cc.MAX_ITEMS and (kinds == items if items else kinds.count(2) >= 2)
    if ends is not None:  # the run alone: chunks (and fills), at element starts
        at = len(wire) - max(ends)
        assert 0 not in kinds and all(s - at in ends for s, _, k in table if k == 2 and s)
    got = pr.run_holder(h, wire, mode)
    assert got[:2] == (status, 1)
    h[0].wg = False  # k_pb2json on the same slot
    try:
        assert pr.run_holder(h, wire, mode) == (status, 0, got[2])
    finally:
        h[0].wg = True
    if status == 0:
        assert json.loads(got[2])["result"]["content"][0]["text"] == text
        if mode & cc.STRUCT:
            assert got[2].endswith(b',"structuredContent":' + text.encode()
                                   + b',"isError":false}}')
        if mode == 0:
            assert pc.same_json(pc.loads(text), pc.loads(pc.oracle_print(h[1], wire)),
                                h[1].DESCRIPTOR)
