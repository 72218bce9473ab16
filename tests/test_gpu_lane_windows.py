"""Lane-window edges of the gfx950 kernels, judged by oracles that are not
the kernel: json, Python's strict UTF-8 decoder, base64 and json_format.

The CPU tier builds the kernels at WAVE=1, where the 64-byte skip_ws window,
the 4-byte-per-lane 256-byte windows (string_end, utf8_span_valid,
wave_copy, put_escaped's clean/dirty/scan paths), the 64-groups-per-pass
put_base64 loop, k_tight_scan and k_compact_out's dword/tail split are all
serial loops (or absent).  The generators live in tests/protojson_corpus.py
and also run on the serial build (test_protojson_surface.py)."""

import pytest

import protojson_corpus as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from ggrmcp_amd.engine.batch import GpuEngine

    return pc.make_env(lambda infos: GpuEngine(infos, device=0))


def test_gpu_string_sweep_all_alignments(env):
    """Lengths around 64/128/256/512/1024 with one special character at the
    edges; raw and \\uXXXX input, bare and enveloped output; four slot
    alignments, byte-identical results."""
    assert pc.check_string_sweep(env) is None


def test_gpu_utf8_defects_at_window_edges(env):
    assert pc.check_utf8(env) is None


def test_gpu_whitespace_runs(env):
    assert pc.check_whitespace(env) is None


def test_gpu_base64_pass_boundaries(env):
    assert pc.check_base64(env) is None


@pytest.mark.parametrize("n", pc.COMPACTION_SIZES)
def test_gpu_compaction_offsets(env, n):
    """k_tight_scan's per-thread chunk changes at 256 and 512 slots; skipped
    and failing slots feed zero/dead lengths into the scan."""
    assert pc.check_compaction(env, n) is None
