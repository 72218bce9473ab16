"""Schemas past 64 fields / 32 oneofs and 5-byte tags on the CPU
(single-lane) build: tests/wide_schema_corpus.py, one test per case id.

Encode runs bare (mode 1) and inside a tools/call envelope (mode 0).  Decode
runs through ``decode_batch(..., wg=False)`` and through the workgroup decode
driver (``wg=True`` with GGRMCP_WG_DEC_MIN=1), flags clear and with
DM_UNPOPULATED; the two must agree with each other and with the oracle.  The
@gpu twin is test_gpu_wide_schema.py.
"""

import os
import struct

import pytest

import wide_schema_corpus as wc
from ggrmcp_amd.engine.hostsim import HostSimEngine
from ggrmcp_amd.engine.tables import (F_ONEOF, FIELD_ENTRY_FMT,
                                      FIELD_ENTRY_SIZE, ONEOF_ID_NONE)


@pytest.fixture(scope="module")
def env():
    return wc.make_env(HostSimEngine)


@pytest.fixture(scope="module")
def wires(env):
    return {"plain": wc.wires(env), "unpop": wc.wires(env, wc.DM_UNPOPULATED)}


@pytest.fixture(scope="module")
def results(env, wires):
    """Every batch of the corpus, run once."""
    out = {
        "accept-encode": wc.run_encode(env, wc.ACCEPT),
        "accept-envelope": wc.run_encode(env, wc.ACCEPT, wc.encode_envelope),
        "reject-encode": wc.run_encode(env, wc.REJECT),
        "reject-envelope": wc.run_encode(env, wc.REJECT, wc.encode_envelope),
    }
    os.environ["GGRMCP_WG_DEC_MIN"] = "1"
    try:
        for name, flags in (("plain", 0), ("unpop", wc.DM_UNPOPULATED)):
            out[f"decode-{name}"] = wc.run_decode(env, wires[name], flags, wg=False)
            out[f"decode-{name}-wg"] = wc.run_decode(env, wires[name], flags, wg=True)
    finally:
        os.environ.pop("GGRMCP_WG_DEC_MIN", None)
    return out


def _ids(cases):
    return [c.id for c in cases]


WIRE_IDS = _ids(wc.ACCEPT) + _ids(wc.HAND_WIRES)


@pytest.mark.parametrize("cid", _ids(wc.ACCEPT))
def test_accept_encode(results, cid):
    assert results["accept-encode"][cid] is None, results["accept-encode"][cid]


@pytest.mark.parametrize("cid", _ids(wc.ACCEPT))
def test_accept_encode_envelope(results, cid):
    assert results["accept-envelope"][cid] is None, results["accept-envelope"][cid]


@pytest.mark.parametrize("cid", _ids(wc.REJECT))
def test_reject_encode(env, results, cid):
    case = next(c for c in wc.REJECT if c.id == cid)
    assert wc.oracle_parse(env, case) is None, \
        "corpus error: the oracle accepts a REJECT payload"
    assert results["reject-encode"][cid] is None, results["reject-encode"][cid]


@pytest.mark.parametrize("cid", _ids(wc.REJECT))
def test_reject_encode_envelope(results, cid):
    assert results["reject-envelope"][cid] is None, results["reject-envelope"][cid]


@pytest.mark.parametrize("form", ["bare", "envelope"])
@pytest.mark.parametrize("case", wc.GO_STRICT, ids=_ids(wc.GO_STRICT))
def test_duplicate_under_both_names_rejected(env, case, form):
    """Proto name + JSON name of one field (rule at wc._dup_names_cases)."""
    encode = wc.encode_direct if form == "bare" else wc.encode_envelope
    enc, _ = encode(env, [case])
    assert int(enc[0]["status"]) != 0


def _check_decode(results, cases, cid, flags):
    i = _ids(cases).index(cid)
    classic, classic_raw = results[f"decode-{flags}"]
    wg, wg_raw = results[f"decode-{flags}-wg"]
    assert classic[cid] is None, classic[cid]
    assert wg[cid] is None, "workgroup driver: " + wg[cid]
    if cases[i].host and {classic_raw[i][0], wg_raw[i][0]} & set(wc.HOST_STATUSES):
        return  # the tagged rule may apply to one path alone
    assert classic_raw[i] == wg_raw[i], (classic_raw[i], wg_raw[i])


@pytest.mark.parametrize("cid", WIRE_IDS)
def test_wires_decode(results, wires, cid):
    _check_decode(results, wires["plain"], cid, "plain")


@pytest.mark.parametrize("cid", [
    c for c in WIRE_IDS if c in wc.UNPOP_WIDE
    or not any(a.id == c and a.msg == wc.MESSAGES[0] for a in wc.ACCEPT)])
def test_wires_decode_unpopulated(results, wires, cid):
    _check_decode(results, wires["unpop"], cid, "unpop")


def test_accept_oracle_verdicts(env):
    for c in wc.ACCEPT + wc.GO_STRICT:
        assert wc.oracle_parse(env, c) is not None, c.id


def test_wires_oracle_verdicts_pinned(env):
    refused = {c.id for c in wc.HAND_WIRES
               if wc.oracle_print(env, c.msg, c.data) is None}
    assert refused == wc.WIRES_ORACLE_REJECTS, \
        sorted(refused ^ wc.WIRES_ORACLE_REJECTS)


def test_corpus_shape(wires):
    """Unique ids; HOST tags on at most one case in eight of each list, each
    quoting a rule docs/KERNELS.md writes down; only index >= 128 and oneofs
    64/65 carry the limit rule."""
    from pathlib import Path

    doc = (Path(__file__).resolve().parent.parent / "docs" / "KERNELS.md").read_text()
    doc = " ".join(doc.split())
    for cases in (wc.ACCEPT, wc.REJECT, wires["plain"], wires["unpop"]):
        assert len({c.id for c in cases}) == len(cases)
        tagged = [c for c in cases if c.host]
        assert len(tagged) * wc.HOST_CAP <= len(cases), [c.id for c in tagged]
        for c in tagged:
            assert c.host in doc, f"{c.id}: rule not in docs/KERNELS.md: {c.host}"
    assert all(c.host is None for c in wc.REJECT)
    limit = {c.id for c in wc.ACCEPT if c.host == wc.LIMIT}
    assert limit == {"alone-128-rstring", "alone-129-map", "oneof-64-alone",
                     "oneof-65-alone", "optional-zero"}


def test_schema_layout(env):
    """What the cases assume about the compiled tables: sorted index = number
    - 1, the kinds at the edge indices, real oneofs 0..65 and no oneof bit
    for the proto3 optionals."""
    kinds = {wc.wide_kind(i) for i in (62, 63, 64, 65, 66, 126, 127, 128, 129)}
    assert {"int32", "string", "leaf", "packed", "rstring", "map"} <= kinds
    assert wc.CHILD_INDEX < 64 and wc.wide_kind(wc.CHILD_INDEX) == "child"
    t = env.engine.tables

    def rows(msg):
        start, count, _wkt, _fl = struct.unpack_from(
            "<iiii", t.msg_table, 16 * t.msg_index[msg])
        return [struct.unpack_from(FIELD_ENTRY_FMT, t.field_table,
                                   FIELD_ENTRY_SIZE * (start + k))
                for k in range(count)]

    wide = rows("w.Wide")
    assert [r[2] for r in wide] == list(range(1, wc.N_WIDE + 1))
    one = rows("w.Oneofs")
    assert len(one) == 2 * wc.N_ONEOFS + 3
    for k, r in enumerate(one[:2 * wc.N_ONEOFS]):
        assert r[9] & F_ONEOF and r[10] == k // 2, (k, r)
    for r in one[2 * wc.N_ONEOFS:]:
        assert not r[9] & F_ONEOF and r[10] == ONEOF_ID_NONE, r
