"""k_pb2json_wg with DM_UNPOPULATED / DM_STRUCTURED on the CPU tier: the
kernel's phases (pb2json_wg.h) driven wave by wave by ``wg_decode_host``,
against the CPU build's classic kernel on the same wires and modes.

``HostSimEngine(infos, wg=True)`` routes every envelope slot of
``GGRMCP_WG_DEC_MIN`` bytes or more to the driver, with the scratch the
engine gives a routed slot.  ``pad`` tells which pass answered: 1 = item
walk, 2 = the in-block classic pass, 0 = not routed."""

import pytest

import protojson_corpus as pc
import unpopulated_corpus as uc
import wg_flags_corpus as wc
from ggrmcp_amd.engine.hostsim import HostSimEngine

FLAGS = uc.DM_UNPOPULATED | uc.DM_STRUCTURED


@pytest.fixture(scope="module")
def classic_envs():
    return uc.make_envs(HostSimEngine)


@pytest.fixture(scope="module")
def wg_envs():
    return uc.make_envs(lambda infos: HostSimEngine(infos, wg=True))


@pytest.fixture()
def low(monkeypatch):
    monkeypatch.setenv("GGRMCP_WG_DEC_MIN", "1")


def _both(classic_envs, wg_envs, cases, flags):
    return wc.run(classic_envs, cases, flags), wc.run(wg_envs, cases, flags)


@pytest.mark.parametrize("flags", wc.FLAG_SETS)
def test_corpora_equal_classic(classic_envs, wg_envs, low, flags):
    """Both corpora, the Any ACCEPT wires and the targeted cases at
    threshold 1: every non-empty wire is routed, (status, bytes) as classic,
    so the set of host escapes is classic's."""
    cases = wc.corpus(classic_envs)
    classic, coop = _both(classic_envs, wg_envs, cases, flags)
    assert not wc.compare(cases, classic, coop, flags)
    routed = [c for c, (_, w) in cases.items() if len(w) >= 1]
    assert all(coop[c][2] in (1, 2) for c in routed)
    assert all(classic[c][2] == 0 for c in cases)
    host = {c for c in cases if classic[c][0] in pc.HOST_STATUSES}
    assert {c for c in cases if coop[c][0] in pc.HOST_STATUSES} == host
    # the item walk, not the classic pass, answers the bulk of them
    assert sum(coop[c][2] == 1 for c in routed) > len(routed) // 2


@pytest.mark.parametrize("flags", wc.FLAG_SETS)
def test_sparse_wide64(classic_envs, wg_envs, low, flags):
    """A few fields of bench.Wide64 present: the gaps go to the fill area,
    not to an item's pad, so the slot stays on the item walk."""
    cases = wc.sparse_wide(classic_envs)
    classic, coop = _both(classic_envs, wg_envs, cases, flags)
    assert not wc.compare(cases, classic, coop, flags)
    s = classic_envs.schema("bench.Wide64")
    for cid, (_, wire) in cases.items():
        st, out, pad, _ = coop[cid]
        assert classic[cid][0] == 0, cid
        assert (st, pad) == (0, 1), (cid, st, pad)
        if flags & uc.DM_STRUCTURED:
            why = uc.verdict(s, wire, 0, wc.raw_slice(out),
                             bool(flags & uc.DM_UNPOPULATED))
            assert why is None, (cid, why)


def test_all_defaults_fit_the_fill_area(classic_envs, wg_envs, low):
    """One present field at either end of bench.Wide64 and x.Rich: the fill
    holds every other default of the message."""
    wide = classic_envs.sink.wide_cls
    cases = {
        "wide:first": ("bench.Wide64", wide(f01_string="a").SerializeToString()),
        "wide:last": ("bench.Wide64", wide(attrs={"k": "v"}).SerializeToString()),
        "rich:first": ("x.Rich", pc.tag(1, 1) + b"\x00" * 6 + b"\xf0\x3f"),
        "rich:last": ("x.Rich", pc.ld(1000, b"z")),
    }
    classic, coop = _both(classic_envs, wg_envs, cases, FLAGS)
    assert not wc.compare(cases, classic, coop, FLAGS)
    for cid, (name, wire) in cases.items():
        st, out, pad, _ = coop[cid]
        assert (st, pad) == (0, 1), (cid, st, pad)
        why = uc.verdict(classic_envs.schema(name), wire, 0, wc.raw_slice(out), True)
        assert why is None, (cid, why)


@pytest.mark.parametrize("flags", wc.FLAG_SETS)
def test_chunk_joins(classic_envs, wg_envs, low, flags):
    cases = wc.chunk_joins(classic_envs)
    classic, coop = _both(classic_envs, wg_envs, cases, flags)
    assert not wc.compare(cases, classic, coop, flags)
    assert all(classic[c][0] == 0 for c in cases)
    assert all(coop[c][2] == 1 for c in cases)


@pytest.mark.parametrize("flags", wc.FLAG_SETS)
def test_hand_assembled_top_level(classic_envs, wg_envs, low, flags):
    cases = wc.hand_wires(classic_envs)
    classic, coop = _both(classic_envs, wg_envs, cases, flags)
    assert not wc.compare(cases, classic, coop, flags)
    for cid in cases:
        assert coop[cid][2] in (1, 2), cid
        if cid in wc.OUT_OF_ORDER:
            assert coop[cid][2] == 2, cid
            assert classic[cid][0] == pc.E_UNSUPPORTED, cid
        else:
            assert classic[cid][0] == 0, (cid, classic[cid][0])


def test_what_leaves_prev_number_alone_takes_the_classic_pass(
        classic_envs, wg_envs, low):
    """The chosen rule for the gap's lower bound: with DM_UNPOPULATED a
    top-level unknown field, foreign wire type or empty packed run sends the
    request to the in-block classic pass; with the flag clear it stays on the
    item walk, as before."""
    cases = {c: v for c, v in wc.hand_wires(classic_envs).items()
             if c not in wc.OUT_OF_ORDER and c.startswith("rich:")}
    plain = wc.run(wg_envs, cases, 0)
    unpop = wc.run(wg_envs, cases, uc.DM_UNPOPULATED)
    assert all(plain[c][2] == 1 for c in cases), plain
    assert all(unpop[c][2] == 2 for c in cases), unpop


@pytest.mark.parametrize("flags", wc.FLAG_SETS)
def test_top_level_any(classic_envs, wg_envs, low, flags):
    cases = wc.any_tops(classic_envs)
    classic, coop = _both(classic_envs, wg_envs, cases, flags)
    assert not wc.compare(cases, classic, coop, flags)
    s = classic_envs.schema("t.Holder")
    for cid, (_, wire) in cases.items():
        st, out, pad, _ = coop[cid]
        assert classic[cid][0] == 0, cid
        assert (st, pad) == (0, 1), (cid, st, pad)
        if flags & uc.DM_STRUCTURED:
            assert uc.verdict(s, wire, 0, wc.raw_slice(out), True) is None, cid


def test_id_shapes_at_every_alignment(classic_envs, wg_envs, low):
    """uc.ENV_IDS behind a leading filler slot one byte longer each run:
    identical across runs, equal to classic, the id replayed verbatim."""
    joins = wc.chunk_joins(classic_envs)
    wires = [w for _, w in list(joins.values())[:len(uc.ENV_IDS)]]
    s, c = wg_envs.schema("bench.Wide64"), classic_envs.schema("bench.Wide64")
    runs = []
    for filler in pc.WIRE_FILLERS:
        outs = uc.run_envelopes(s, wg_envs.sink.sink_tool, [filler] + wires,
                                [0] + uc.ENV_IDS, FLAGS)
        assert outs[0][0] == 0
        runs.append(outs[1:])
    assert pc._first_diff(runs) is None
    ref = uc.run_envelopes(c, classic_envs.sink.sink_tool,
                           [pc.WIRE_FILLERS[0]] + wires, [0] + uc.ENV_IDS, FLAGS)
    assert runs[0] == ref[1:]
    for rid, (status, out) in zip(uc.ENV_IDS, runs[0]):
        assert status == 0
        assert uc.check_envelope(out, uc.id_token(rid)) is None


def test_skipped_and_failing_neighbours(classic_envs, wg_envs, low):
    """A skipped slot and a failing wire between routed slots."""
    joins = list(wc.chunk_joins(classic_envs).values())
    good = joins[0][1]
    wires = [good, None, pc.ld(1, b"bad\x80"), joins[1][1], good]
    skip = [False, False, False, False, True]
    s, c = wg_envs.schema("bench.Wide64"), classic_envs.schema("bench.Wide64")
    got = uc.run_envelopes(s, wg_envs.sink.sink_tool, wires, list(range(5)),
                           FLAGS, skip=skip)
    ref = uc.run_envelopes(c, classic_envs.sink.sink_tool, wires,
                           list(range(5)), FLAGS, skip=skip)
    assert got == ref
    assert [st for st, _ in got] == [0, 0, pc.E_UNSUPPORTED, 0, 0]
    assert got[1][1] is None and got[4][1] is None


def test_default_threshold_routes_only_large(classic_envs, wg_envs, monkeypatch):
    monkeypatch.delenv("GGRMCP_WG_DEC_MIN", raising=False)
    cases = dict(list(wc.chunk_joins(classic_envs).items())[:1])
    m = classic_envs.sink.wide_cls(f01_string="s" * 500)
    m.attrs.update(wc._attrs(20_000))
    cases["big"] = ("bench.Wide64", m.SerializeToString())
    classic, coop = _both(classic_envs, wg_envs, cases, FLAGS)
    assert not wc.compare(cases, classic, coop, FLAGS)
    assert [coop[c][2] for c in cases] == [0, 1]


def test_unextended_final_arena_overflows_cleanly(wg_envs, low):
    """The structured envelope with final_cap alone: E_OVERFLOW before any
    write, for the item walk as for the classic pass (decode_wg with the
    final offsets of an unstructured batch)."""
    import numpy as np

    from ggrmcp_amd.engine.batch import DECODE_DTYPE, _offsets
    from ggrmcp_amd.engine.hostsim import WG_DEC_EXTRA, WG_DEC_FILL

    s = wg_envs.schema("bench.Wide64")
    m = wg_envs.sink.wide_cls(f01_string="s" * 900)
    m.attrs.update(wc._attrs(9_000))
    good = m.SerializeToString()
    unknown = good + pc.tag(900, 0) + b"\x01"    # unknown field: classic pass
    wires = [good, unknown]
    enc, _ = s.engine.encode_batch(
        uc.envelope_bodies(wg_envs.sink.sink_tool, [1, 2]), mode=0)
    lens = [len(w) for w in wires]
    scratch = _offsets([n * 8 + 1024 + WG_DEC_EXTRA + WG_DEC_FILL for n in lens],
                       align=16)
    # JSON of ~len bytes twice plus the framing does not fit 1.25x the wire
    final = _offsets([n + n // 4 for n in lens], align=16)
    raw, _ = s.engine._eng.decode_wg(
        b"".join(wires), _offsets(lens), scratch, final,
        np.asarray([s.idx, s.idx], dtype=np.int32),
        np.asarray([2, 2], dtype=np.int32), FLAGS)
    res = np.frombuffer(raw.tobytes(), dtype=DECODE_DTYPE)
    assert [int(r["status"]) for r in res] == [pc.E_OVERFLOW, pc.E_OVERFLOW]
    assert [int(r["pad"]) for r in res] == [1, 2]
    assert all(int(r["out_len"]) == 0 for r in res)
