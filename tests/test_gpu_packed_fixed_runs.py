"""Packed fixed-width runs on gfx950: the 64-lane windows of
``emit_packed_fixed`` (load, format, wave scan of unequal lengths, stores)
against the CPU build's bytes and status, and against ``json_format`` by
parsed value.  The CPU build runs the same code one element per window."""

import pytest

import packed_runs_corpus as pr
import protojson_corpus as pc

pytestmark = pytest.mark.gpu

UNPOP, RO = pr.DM_UNPOPULATED, pr.DM_REORDER


def _gpu(infos):
    from ggrmcp_amd.engine.batch import GpuEngine

    return GpuEngine(infos, device=0)


def _cpu(infos):
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return HostSimEngine(infos, wg=True)


@pytest.fixture(scope="module")
def envs():
    return pc.make_env(_gpu), pc.make_env(_cpu)


@pytest.fixture(scope="module")
def holders():
    return pr.make_holder(_gpu), pr.make_holder(_cpu)


@pytest.mark.parametrize("mode", [1, 0, 1 | UNPOP, 0 | UNPOP])
def test_every_kind_and_run_length(envs, mode):
    """Run lengths around one and two windows, six kinds, texts of 1 to 24
    bytes, at four slot alignments: the CPU build's bytes, status 0."""
    gpu, cpu = envs
    wires = pr.device_wires()
    for filler in range(4):
        got = pr.run_batch(gpu, wires, mode, filler)
        assert [g[0] for g in got] == [0] * len(wires)
        assert got == pr.run_batch(cpu, wires, mode, filler), filler


def test_oracle_values(envs):
    gpu, _ = envs
    wires = pr.device_wires()
    cases = [pc.Case(str(i), w) for i, w in enumerate(wires)]
    for mode in (1, 0):
        bad = {k: v for k, v in pc.run_decode(gpu, cases, wires, mode).items() if v}
        assert not bad, bad


@pytest.mark.parametrize("n", [1, 257])
def test_batch_sizes(envs, n):
    """``n`` slots, each a packed run and no filler; the lone slot of the
    1-slot batch is the 129-element double run (three windows)."""
    gpu, cpu = envs
    w = pr.device_wires()
    at = pr.RUN_LENGTHS.index(129)
    wires = ((w[at:] + w[:at]) * 5)[:n]
    got = pr.run_batch(gpu, wires, 1)
    assert len(got) == n and all(g[0] == 0 and g[2] for g in got)
    assert got == pr.run_batch(cpu, wires, 1)


@pytest.mark.parametrize("name,mode,pads", [("nested", 0, (1, 2)), ("top", 0, (1, 2)),
                                            ("descending", 0 | RO, (3,))])
def test_workgroup_and_reorder_paths(holders, name, mode, pads):
    """A run inside a nested message and one at the top of a >= 16 KB
    response through k_pb2json_wg; descending fields through k_pb_reorder."""
    gpu, cpu = holders
    wire = pr.holder_wires(gpu[1])[name]
    status, pad, out = pr.run_holder(gpu, wire, mode)
    assert status == 0 and pad in pads
    assert (status, pad, out) == pr.run_holder(cpu, wire, mode)
    text = pc.loads(out.decode())["result"]["content"][0]["text"]
    assert pc.same_json(pc.loads(text), pc.loads(pc.oracle_print(gpu[1], wire)),
                        gpu[1].DESCRIPTOR)


@pytest.mark.parametrize("kind,nbytes", pr.BAD_BODIES)
def test_ragged_run_is_parse_error(envs, kind, nbytes):
    wire = pc.ld(pc.F[f"r_{kind}"], bytes(nbytes))
    assert [g[0] for g in pr.run_batch(envs[0], [wire], 1)] == [pr.E_PARSE]


def test_overflow_at_the_second_window(envs):
    """65 elements into a slot that holds the first window and ten bytes:
    E_OVERFLOW; the slot that holds it all to the byte prints the CPU
    build's bytes.  The status is what is judged: the scratch region is not
    handed back, so a store ahead of the check would not show here (the code
    compares the wave-uniform total with the slot before any lane stores)."""
    gpu, cpu = envs
    wire = pr.packed("double", pr.OVERFLOW_RUN)
    status, full = pr.decode_slot(cpu, wire, 4096)
    assert status == 0
    last = pr.elements(full.decode(), "double")[-1]
    assert pr.decode_slot(gpu, wire, len(full)) == (0, full)
    tight = len(full) - len("," + last + "]}") + 10
    assert pr.decode_slot(gpu, wire, tight) == (pr.E_OVERFLOW, None)
