"""Packed varint runs on the CPU build (WAVE=1, a window is one element):
``emit_packed_varint`` (pb2json.hip) against texts built in plain Python,
byte for byte.  ``test_gpu_packed_varint_runs.py`` holds the device build to
this one."""

import json

import pytest

import packed_runs_corpus as pr
import packed_varint_corpus as pv
from test_packed_fixed_runs import env  # noqa: F401


@pytest.mark.parametrize("mode", [1, 0])
def test_every_kind_and_run_length(env, mode):
    """Four slot alignments, bare and in the envelope."""
    wires, want = pv.device_cases()
    for filler in range(4):
        got = pr.run_batch(env, wires, mode, filler)
        assert [g[0] for g in got] == [0] * len(wires)
        outs = [g[2] if mode else
                json.loads(g[2])["result"]["content"][0]["text"].encode()
                for g in got]
        assert outs == want, filler


@pytest.mark.parametrize("wire,want", pv.EXACT)
def test_encodings_and_mixes(env, wire, want):
    assert pr.run_batch(env, [wire], 1) == [(0, 0, want)]


@pytest.mark.parametrize("kind,v,n", pv.FILL)
def test_window_fill(kind, v, n):
    """One element per window on this build; the probe does not exist on the
    parent commit."""
    from ggrmcp_amd.engine.hostsim import load_module

    status, text, windows = load_module().packed_varint_probe(
        kind, pv.body(kind, [v] * n), 16384)
    assert (status, text) == (0, pv.texts(kind, [v] * n).encode())
    assert windows == [1] * n


@pytest.mark.parametrize("wire", pv.MALFORMED)
def test_malformed_is_parse_error(env, wire):
    assert [g[0] for g in pr.run_batch(env, [wire], 1)] == [pr.E_PARSE]


def test_overflow_at_the_second_window(env):
    """65 elements: a region that holds the whole text to the byte prints it;
    one that holds the first 64 and ten bytes more ends in E_OVERFLOW."""
    wire = pv.packed("int64", pv.OVERFLOW_RUN)
    full = pv.expected("int64", pv.OVERFLOW_RUN)
    assert pr.decode_slot(env, wire, len(full)) == (0, full)
    tight = len(full) - len(',"%d"]}' % pv.OVERFLOW_RUN[-1]) + 10
    assert pr.decode_slot(env, wire, tight) == (pr.E_OVERFLOW, None)
