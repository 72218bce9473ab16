"""Type table of the GPU table compiler (google.protobuf.Any resolution)."""

import struct

import any_corpus as ac
from examples.protos import ALL_FDPS
from ggrmcp_amd.descriptors.loader import build_pool, extract_method_infos
from ggrmcp_amd.engine import tables as T


def _compile():
    _, infos = ac.make_infos()
    return T.compile_tables(infos)


def _is_map_entry(name):
    pool, _ = ac.make_infos()
    return pool.FindMessageTypeByName(name).GetOptions().map_entry


def _entries(ct):
    n = len(ct.type_table) // T.TYPE_ENTRY_SIZE
    return [struct.unpack_from(T.TYPE_ENTRY_FMT, ct.type_table, i * T.TYPE_ENTRY_SIZE)
            for i in range(n)]


def test_types_known_only_through_any_are_compiled():
    ct = _compile()
    # t.Orphan is referenced by no field, u.Other lives in an imported file
    for name in ("t.Holder", "t.Leaf", "t.Orphan", "t.Deep", "u.Other",
                 "google.protobuf.Any", "google.protobuf.Duration",
                 "google.protobuf.Int64Value", "google.protobuf.Struct"):
        assert name in ct.msg_index, name
    assert "v.Stranger" not in ct.msg_index
    assert len(ct.msg_table) == ct.n_msgs * T.MSG_ENTRY_SIZE
    assert ct.n_msgs == len(ct.msg_index)


def test_type_table_entries():
    ct = _compile()
    assert len(ct.type_table) % T.TYPE_ENTRY_SIZE == 0
    assert T.TYPE_ENTRY_SIZE % 8 == 0        # the u64 hash stays 8-byte aligned
    rows = _entries(ct)
    by_idx = {idx: name for name, idx in ct.msg_index.items()}
    listed = set()
    for h, idx, off, ln, pad, pad2 in rows:
        name = ct.name_blob[off:off + ln].decode()
        assert name == by_idx[idx]
        assert h == T.fnv1a64(name.encode())
        assert (pad, pad2) == (0, 0)
        listed.add(name)
    # one entry per message, map entries excluded
    assert len(rows) == len(listed)
    assert listed == {n for n in ct.msg_index if not _is_map_entry(n)}
    assert "t.Holder.MaEntry" in ct.msg_index and "t.Holder.MaEntry" not in listed
    hashes = [r[0] for r in rows]
    assert hashes == sorted(hashes)


def test_compiling_twice_gives_equal_blobs():
    a, b = _compile(), _compile()
    assert len(a.blobs()) == 7 and a.blobs()[6] == a.type_table
    assert a.blobs() == b.blobs()
    assert a.checksum() == b.checksum()
    assert a.msg_index == b.msg_index


def test_checksum_covers_the_type_table():
    a = _compile()
    before = a.checksum()
    a.type_table = a.type_table[:-1] + bytes([a.type_table[-1] ^ 1])
    assert a.checksum() != before


# FNV-1a64 of the six blobs the compiler produced for examples.protos.ALL_FDPS
# (compat tool names) BEFORE the type table existed, taken from that commit.
_PARENT_BLOB_HASHES = [
    0x5CFF39A0F3669322, 0x00A0FFCC985D2DC1, 0x48C2A43A7E4FF656,
    0x182C0BA4A0962D51, 0x54A40DF99D08813D, 0xCAA47A1A766EF1B8,
]
_PARENT_N_MSGS = 9
_PARENT_MSG_INDEX_HASH = 0x83C04AC720D8CFA0


def test_tables_without_any_are_unchanged():
    """No tool of the example schemas reaches an Any: the six older blobs,
    n_msgs and msg_index are what the compiler gave before (pinned hashes,
    not a re-run with the new step disabled), and type_table is empty."""
    pool = build_pool(ALL_FDPS)
    infos = {m.tool_name(): m for m in extract_method_infos(ALL_FDPS, pool)}
    ct = T.compile_tables(infos)
    assert "google.protobuf.Any" not in ct.msg_index
    assert ct.type_table == b""
    assert [T.fnv1a64(b) for b in ct.blobs()[:6]] == _PARENT_BLOB_HASHES
    assert ct.n_msgs == _PARENT_N_MSGS
    assert T.fnv1a64(repr(sorted(ct.msg_index.items())).encode()) \
        == _PARENT_MSG_INDEX_HASH
