"""Packed arrays in the workgroup encode kernel, CPU build: the chunk items
(``wg_pack_chunk``, kinds 4 and 5) and the phase-C length backfill
(``wg_pack_backfill``) through ``HostEngine.encode_packed_chunks``.  The kernel
itself is not in the CPU build; test_gpu_wg_packed_encode.py runs it."""

import pytest

import packed_encode_corpus as pe
import protojson_corpus as pc
import wg_packed_encode_cases as wp
from ggrmcp_amd.engine.hostsim import HostSimEngine, load_module

LEN_SLOT_MAX = (1 << 21) - 1   # common.h


@pytest.fixture(scope="module")
def env():
    return pc.make_env(HostSimEngine)


def chunks(env, kind, text, cuts):
    return env.engine.encode_packed_chunks(
        env.sink_idx, wp.field_index(kind), text.encode(), cuts)


@pytest.mark.parametrize("kind", wp.KINDS)
def test_cut_array_equals_the_uncut_encode(env, kind):
    el = [wp.ELEMENT[kind](i) for i in range(wp.HOST_ELEMENTS)]
    text = ",".join(el)
    doc = '{"%s":[%s]}' % (wp.field_name(kind), text)
    res, pbs = env.engine.encode_batch([doc.encode()], mode=1,
                                       msg_indices=[env.sink_idx], enforce=False)
    assert int(res[0]["status"]) == 0
    assert pbs[0] == wp.record(kind, el)
    for n in wp.CUT_COUNTS:
        cuts = wp.comma_cuts(text, n)
        assert len(set(cuts)) == n
        assert chunks(env, kind, text, cuts) == (0, pbs[0]), (kind, n)


def test_last_element_of_a_chunk_goes_through_the_window(env):
    """Subnormals, DBL_MAX and 35-digit texts: the serial element sends them
    to the host, so a chunk must not leave its last element to it."""
    text = ",".join(pe.EXTREMES_65)
    for cuts in ([], wp.comma_cuts(text, 7), [i for i, ch in enumerate(text) if ch == ","]):
        assert chunks(env, "double", text, cuts) == (0, pe.ref_wire("double", pe.EXTREMES_65))


@pytest.mark.parametrize("text,cuts", [
    ("1,,2", [1, 2]),        # an empty chunk between two cuts
    ("1,2,", [3]),           # a trailing comma on the cut: empty last chunk
    (",1,2", [0]),           # empty first chunk
    ("1, \t,2", [1, 4]),     # whitespace only
    ("1,2,,3", [1]),         # two commas inside the second chunk
    ("1,2,", [1]),           # a chunk that ends in a comma
    ("1,2],[3,4", [4]),      # a ']' inside a chunk
    ("1,2]", []),            # ... which the window consumes
    ("1,2 x", [1]),          # stops before the span end
])
def test_bad_chunks_are_refused(env, text, cuts):
    # int32 goes through the window first, enum through the serial loop alone
    for kind in ("int32", "enum"):
        status, wire = chunks(env, kind, text, cuts)
        assert status != 0 and wire == b"", kind


def test_chunk_overflow_is_refused(env):
    # 8 bytes of wire for 2 of text: 808 bytes into an item of 408
    text = ",".join(["0"] * 100)
    assert chunks(env, "double", text, [])[0] == pc.E_OVERFLOW
    assert chunks(env, "double", text, wp.comma_cuts(text, 1))[0] == pc.E_OVERFLOW
    assert chunks(env, "int32", text, [])[0] == 0


def test_backfill_sums_and_refuses_past_the_slot():
    mod = load_module()
    number = pc.F["r_double"]
    head = 1 + 3             # one-byte tag, the length slot
    assert mod.wg_pack_backfill(number, [head + 5, 300, 2]) == \
        (True, bytes([0x80 | 307 & 0x7F, 0x80 | 307 >> 7, 0]))
    full = [head + 4096] + [4096] * 510 + [4095]
    assert sum(full) - head == LEN_SLOT_MAX
    ok, slot = mod.wg_pack_backfill(number, full)
    assert ok and slot == b"\xff\xff\x7f"
    full[-1] += 1
    assert mod.wg_pack_backfill(number, full)[0] is False
    assert mod.wg_pack_backfill(2 ** 29 - 1, [5 + 3 + 1])[0] is True  # 5-byte tag
