"""Packed fixed-width runs on the CPU build (WAVE=1): the exact
shortest-digits generator (csrc/fp_shortest.h) and the run printer
(pb2json.hip ``emit_packed_fixed``), judged by ``repr``, ``struct`` and
``json_format``.  ``test_gpu_packed_fixed_runs.py`` holds the device build to
this one."""

import struct

import pytest

import packed_runs_corpus as pr
import protojson_corpus as pc


@pytest.fixture(scope="module")
def env():
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return pc.make_env(HostSimEngine)


def _decode_runs(env, kind, values, chunk=200, wire=pr.packed):
    """``values`` in runs of ``chunk`` -> their element texts; status 0."""
    parts = [values[i:i + chunk] for i in range(0, len(values), chunk)]
    dec, outs = env.engine.decode_batch([wire(kind, p) for p in parts],
                                        [env.sink_idx] * len(parts), mode=1)
    assert [int(r["status"]) for r in dec] == [0] * len(parts)
    texts = [t for o in outs for t in pr.elements(o.decode(), kind)]
    assert len(texts) == len(values)
    return texts


def test_every_binary_exponent_double(env):
    """Mantissa 0, 1, all-ones and random at biased exponents 0..2046: the
    text parses back to the value and carries exactly repr's digits."""
    for v, text in zip(pr.DOUBLES, _decode_runs(env, "double", pr.DOUBLES)):
        assert float(text) == v, (v, text)
        assert pr.sig_digits(text) == pr.sig_digits(repr(v)), (v, text)


def test_every_binary_exponent_float(env):
    for v, text in zip(pr.FLOATS, _decode_runs(env, "float", pr.FLOATS)):
        assert struct.pack("<f", float(text)) == struct.pack("<f", v), (v, text)
        assert pr.sig_digits(text) == pr.sig_digits(pr.shortest_float32(v)), (v, text)


def test_packed_equals_unpacked(env):
    """Where the singular emitter already prints the shortest digits, a
    packed run is the same bytes as the same values one by one."""
    vals = pr.random_doubles(4000, 7) + pr.LAYOUT_SWEEP
    assert (_decode_runs(env, "double", vals)
            == _decode_runs(env, "double", vals, wire=pr.unpacked))


@pytest.mark.parametrize("kind", ["fixed32", "sfixed32", "fixed64", "sfixed64",
                                  "double", "float"])
def test_integer_kinds_and_nonfinite(env, kind):
    vals = pr.INT_EDGES.get(kind, pr.NONFINITE)
    wire = pr.packed(kind, vals)
    res = pc.run_decode(env, [pc.Case(kind, wire)], [wire])
    assert res[kind] is None, res[kind]


@pytest.mark.parametrize("kind,nbytes", pr.BAD_BODIES)
def test_ragged_run_is_parse_error(env, kind, nbytes):
    wire = pc.ld(pc.F[f"r_{kind}"], bytes(nbytes))
    dec, _ = env.engine.decode_batch([wire], [env.sink_idx], mode=1)
    assert int(dec[0]["status"]) == pr.E_PARSE


def test_overflow_at_the_second_window(env):
    """65 elements: with room for all the slot prints; with room for the
    first 64 and ten bytes more it ends in E_OVERFLOW."""
    wire = pr.packed("double", pr.OVERFLOW_RUN)
    status, full = pr.decode_slot(env, wire, 4096)
    assert status == 0
    last = pr.elements(full.decode(), "double")[-1]
    assert pr.decode_slot(env, wire, len(full)) == (0, full)
    tight = len(full) - len("," + last + "]}") + 10
    assert pr.decode_slot(env, wire, tight) == (pr.E_OVERFLOW, None)
