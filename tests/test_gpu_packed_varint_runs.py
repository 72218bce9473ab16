"""Packed varint runs on gfx950: the 64-lane windows of ``emit_packed_varint``
(terminator ballots, rank-select, per-lane fold and format, wave scan of
unequal lengths, stores) against texts built in plain Python and against the
CPU build's ``(status, pad, bytes)``; the window fill through the probe."""

import pytest

import packed_runs_corpus as pr
import packed_varint_corpus as pv
import protojson_corpus as pc
from test_gpu_packed_fixed_runs import _cpu, _gpu, envs  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def holders():
    return pv.make_holder(_gpu), pv.make_holder(_cpu)


@pytest.mark.parametrize("mode", [1, 0])
def test_every_kind_and_run_length(envs, mode):
    """Four slot alignments, bare and enveloped: the CPU build's result."""
    gpu, cpu = envs
    wires, want = pv.device_cases()
    for filler in range(4):
        got = pr.run_batch(gpu, wires, mode, filler)
        assert [g[0] for g in got] == [0] * len(wires)
        assert got == pr.run_batch(cpu, wires, mode, filler), filler
        assert not mode or [g[2] for g in got] == want


@pytest.mark.parametrize("n", [1, 257])
def test_batch_sizes(envs, n):
    """``n`` slots; the lone slot is the 129-element int32 run."""
    wires, want = pv.device_cases()
    at = pv.RUN_LENGTHS.index(129)
    pick = lambda xs: ((xs[at:] + xs[:at]) * 5)[:n]  # noqa: E731
    assert pr.run_batch(envs[0], pick(wires), 1) == [(0, 0, w) for w in pick(want)]


@pytest.mark.parametrize("wire,want", pv.EXACT)
def test_encodings_and_mixes(envs, wire, want):
    assert pr.run_batch(envs[0], [wire], 1) == [(0, 0, want)]


@pytest.mark.parametrize("kind,v,n", pv.FILL)
def test_window_fill(kind, v, n):
    """Ten-byte elements fill as many lanes as lie whole in one stretch."""
    from ggrmcp_amd import ops

    mod = ops.load()
    status, text, windows = mod.packed_varint_probe(kind, pv.body(kind, [v] * n), 16384)
    assert (status, text) == (0, pv.texts(kind, [v] * n).encode())
    assert sum(windows) == n and max(windows) <= 64
    per = min(64, mod.PV_STRETCH // len(pc.vi(v)))
    assert windows[:-1] == [per] * (len(windows) - 1) and windows[-1] <= per
    assert len(pc.vi(v)) > 1 or windows == [64, 64, 64, 8]


@pytest.mark.parametrize("wire", pv.MALFORMED)
def test_malformed_is_parse_error(envs, wire):
    assert [g[0] for g in pr.run_batch(envs[0], [wire], 1)] == [pr.E_PARSE]


def test_overflow_at_the_second_window(envs):
    """The region that holds all 65 texts to the byte prints them; the first
    window and ten bytes: E_OVERFLOW (the status alone is judged)."""
    wire = pv.packed("int64", pv.OVERFLOW_RUN)
    full = pv.expected("int64", pv.OVERFLOW_RUN)
    assert pr.decode_slot(envs[0], wire, len(full)) == (0, full)
    tight = len(full) - len(',"%d"]}' % pv.OVERFLOW_RUN[-1]) + 10
    assert pr.decode_slot(envs[0], wire, tight) == (pr.E_OVERFLOW, None)


@pytest.mark.parametrize("name,mode,pads", [("nested", 0, (1, 2)), ("top", 0, (1, 2)),
                                            ("descending", pr.DM_REORDER, (3,))])
def test_workgroup_and_reorder_paths(holders, name, mode, pads):
    """>= 16 KB through k_pb2json_wg; descending fields through k_pb_reorder."""
    gpu, cpu = holders
    wire = pv.holder_wires(gpu[1])[name]
    status, pad, out = pr.run_holder(gpu, wire, mode)
    assert status == 0 and pad in pads
    assert (status, pad, out) == pr.run_holder(cpu, wire, mode)
    text = pc.loads(out.decode())["result"]["content"][0]["text"]
    assert pc.same_json(pc.loads(text), pc.loads(pc.oracle_print(gpu[1], wire)),
                        gpu[1].DESCRIPTOR)
