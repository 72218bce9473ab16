"""k_pack_out's offset arithmetic on the CPU build.

``_hostsim.pack_offsets`` runs the kernel's own functions (pb2json.hip
pack_partial / pack_place, summed over its 256 thread indices) over a batch
of out_len values.  The reference is a plain Python prefix sum of the
4-aligned lengths."""

import numpy as np
import pytest

from ggrmcp_amd.engine.hostsim import load_module

LENGTHS = (0, 1, 3, 4, 5, 1023, 1024)
SIZES = (1, 2, 255, 256, 257, 513, 4096)
BIG_CAP = 1 << 30


@pytest.fixture(scope="module")
def pack():
    return load_module().pack_offsets


def prefix(lens):
    offs, acc = [], 0
    for n in lens:
        offs.append(acc)
        acc += (n + 3) & ~3
    return offs, acc


def check(pack, lens, cap):
    offs, writes, total = pack(np.asarray(lens, dtype=np.uint32), cap)
    want, acc = prefix(lens)
    assert total == acc
    assert offs.tolist() == want
    # all slots write, or (the batch does not fit) none does
    assert writes.tolist() == [acc <= cap] * len(lens)
    return acc


@pytest.mark.parametrize("n", SIZES)
def test_every_length_in_every_position(pack, n):
    """Seven rotations of the length cycle: across them each position of the
    batch holds each of the seven lengths once."""
    for shift in range(len(LENGTHS)):
        lens = [LENGTHS[(i + shift) % len(LENGTHS)] for i in range(n)]
        check(pack, lens, BIG_CAP)


@pytest.mark.parametrize("n", SIZES)
def test_all_zero(pack, n):
    assert check(pack, [0] * n, BIG_CAP) == 0
    assert check(pack, [0] * n, 0) == 0


def test_empty_batch(pack):
    offs, writes, total = pack(np.zeros(0, dtype=np.uint32), 16)
    assert (len(offs), len(writes), total) == (0, 0, 0)


@pytest.mark.parametrize("n", (1, 2, 257, 4096))
def test_total_at_and_past_the_cap(pack, n):
    """total == dst_cap packs; one byte more (a whole aligned word) does
    not, and then no slot writes."""
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(n - 1)] + [1021]
    _, acc = prefix(lens)
    assert check(pack, lens, acc) == acc
    # the same batch against a cap one byte smaller: total == dst_cap + 1
    assert check(pack, lens, acc - 1) == acc
    # the last slot grows by one byte past its aligned end
    lens[-1] = 1025
    _, acc2 = prefix(lens)
    assert acc2 > acc
    offs, writes, total = pack(np.asarray(lens, dtype=np.uint32), acc)
    assert total == acc2 > acc and not writes.any()
    # an unaligned tail that still ends inside the cap fits exactly
    check(pack, [5, 3], 8)
    offs, writes, total = pack(np.asarray([5, 5], dtype=np.uint32), 15)
    assert total == 16 and not writes.any()


@pytest.mark.parametrize("lens", [
    [0x80000000, 0x80000000],                 # 32-bit sum wraps to 0
    [0xFFFFFFFC, 4, 4],                       # wraps to 4
    [0xFFFFFFFF, 1],                          # aligned length itself is 2^32
    [0x40000000] * 9,                         # wraps twice
    [1 << 20] * 4096,                         # exactly 2^32
    [0x7FFFFFFF] * 513,
])
def test_32bit_wrap_reports_overflow(pack, lens):
    cap = 0xFFFFFFF0  # the largest dst_cap the engine passes
    offs, writes, total = pack(np.asarray(lens, dtype=np.uint32), cap)
    _, acc = prefix(lens)
    assert acc >= 1 << 32
    assert total > cap, "a wrapped sum must not look like a small total"
    assert not writes.any()
    # offsets that still fit 32 bits are exact; the rest saturate
    want, _ = prefix(lens)
    assert offs.tolist() == [min(w, 0xFFFFFFFF) for w in want]
