"""Packed arrays split across the waves of ``k_json2pb_wg``, gfx950: chunk
items of kinds 4 and 5, the length backfill of phase C and the multi-wave
scanner past 512 commas one level down.  Wire against the Python reference
(``wg_packed_encode_cases.record``), the protojson oracle and the classic
kernel; refusals against the CPU build's result record."""

import os
from contextlib import contextmanager

import pytest
from google.protobuf import json_format

import protojson_corpus as pc
import wg_packed_encode_cases as wp
import wide_schema_corpus as wc
from ggrmcp_amd.engine.batch import SR_WG_CLASSIC, SR_WG_ITEMS, SR_WG_PACK

pytestmark = pytest.mark.gpu
PATH_BITS = SR_WG_ITEMS | SR_WG_CLASSIC | SR_WG_PACK


def _gpu(infos):
    from ggrmcp_amd.engine.batch import GpuEngine

    return GpuEngine(infos, device=0)


def _cpu(infos):
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return HostSimEngine(infos)


@pytest.fixture(scope="module")
def envs():
    return pc.make_env(_gpu), pc.make_env(_cpu)


@contextmanager
def _setenv(**kw):
    os.environ.update(kw)
    try:
        yield
    finally:
        for k in kw:
            os.environ.pop(k, None)


def run(env, docs, mw, wg_min="1"):
    """The documents as tools/call arguments through k_json2pb_wg and through
    the classic kernel: ([result], [wire]) of each."""
    bodies = [wc.envelope(env.sink_tool, d, i) for i, d in enumerate(docs)]
    with _setenv(GGRMCP_WG_ENC_MIN=wg_min, GGRMCP_MW_SCAN=str(mw)):
        enc, pbs = env.engine.encode_batch(bodies, mode=0, enforce=False)
    with _setenv(GGRMCP_WG_ENC_MIN="1000000000"):
        cenc, cpbs = env.engine.encode_batch(bodies, mode=0, enforce=False)
    return bodies, enc, pbs, cenc, cpbs


def same_record(r, cr):
    return all(int(r[k]) == int(cr[k])
               for k in ("status", "err_pos", "aux", "id_len", "tool_idx"))


def oracle_bytes(env, doc):
    return json_format.Parse(doc, env.sink_cls()).SerializeToString(deterministic=True)


@pytest.mark.parametrize("mw", [0, 1])
@pytest.mark.parametrize("kind", wp.KINDS)
def test_split_array_accepts(envs, kind, mw):
    gpu, _ = envs
    cases = wp.accept_docs(kind)
    _, enc, pbs, cenc, cpbs = run(gpu, [d for _, d, _ in cases], mw)
    for (shape, doc, el), r, pb, cr, cpb in zip(cases, enc, pbs, cenc, cpbs):
        assert int(r["status"]) == 0 and same_record(r, cr), shape
        assert int(r["flags"]) & PATH_BITS == SR_WG_ITEMS | SR_WG_PACK, shape
        assert int(cr["flags"]) & PATH_BITS == 0, shape
        assert pb == cpb, shape
        rec = wp.record(kind, el)
        assert pb == rec if shape in ("alone", "whitespace", "quoted") \
            else rec in pb, shape
        msg = gpu.sink_cls.FromString(pb)
        assert msg.SerializeToString(deterministic=True) == oracle_bytes(gpu, doc), shape


@pytest.mark.parametrize("which", [0, 1], ids=["map", "messages"])
def test_cap_lift_without_packed_data(envs, which):
    gpu, _ = envs
    doc = wp.CAP_LIFT_DOCS[which]
    _, enc, pbs, cenc, cpbs = run(gpu, [doc], 1)
    assert int(enc[0]["status"]) == 0 and same_record(enc[0], cenc[0])
    assert int(enc[0]["flags"]) & PATH_BITS == SR_WG_ITEMS
    assert pbs[0] == cpbs[0]
    assert gpu.sink_cls.FromString(pbs[0]).SerializeToString(deterministic=True) \
        == oracle_bytes(gpu, doc)


@pytest.mark.parametrize("mw", [0, 1])
def test_refusals_take_the_classic_pass(envs, mw):
    gpu, cpu = envs
    bodies, enc, pbs, cenc, _ = run(gpu, [d for _, d, _ in wp.REFUSALS], mw)
    want, _ = cpu.engine.encode_batch(bodies, mode=0, enforce=False)
    for (cid, doc, oracle_refuses), r, pb, w in zip(wp.REFUSALS, enc, pbs, want):
        if oracle_refuses:
            with pytest.raises(json_format.ParseError):
                json_format.Parse(doc, gpu.sink_cls())
        assert int(w["status"]) != 0, cid
        assert int(r["flags"]) & PATH_BITS == SR_WG_CLASSIC, cid
        assert [int(r[k]) for k in ("status", "err_pos", "aux")] == \
            [int(w[k]) for k in ("status", "err_pos", "aux")], cid
        assert pb is None, cid
    assert int(want[-1]["status"]) == pc.E_OVERFLOW


@pytest.mark.parametrize("n", [1, 9])
def test_batch_of_mixed_slots(envs, n):
    """Split, unsplit, failing and below-threshold slots side by side, so a
    neighbour's scratch region lies next to every split array's."""
    gpu, _ = envs
    split = [wp.accept_docs(k)[0] for k in ("double", "int32", "bool")]
    pad = ",".join(['"%s"' % ("QUJD" * 25)] * 100)
    # the short array comes last: under 2048 bytes to go, it is a member item
    unsplit = '{"rBytes":[%s],"rInt32":[1,2,3]}' % pad
    small = '{"rDouble":[1.5,"NaN",-0.0],"optStr":"s"}'
    docs = [split[0][1], small, wp.REFUSALS[1][1], unsplit, split[1][1],
            wp.REFUSALS[-1][1], small, split[2][1], unsplit][:n]
    want_bits = [SR_WG_ITEMS | SR_WG_PACK, 0, SR_WG_CLASSIC, SR_WG_ITEMS,
                 SR_WG_ITEMS | SR_WG_PACK, SR_WG_CLASSIC, 0,
                 SR_WG_ITEMS | SR_WG_PACK, SR_WG_ITEMS][:n]
    _, enc, pbs, cenc, cpbs = run(gpu, docs, 1, wg_min="4096")
    for i, (r, pb, cr, cpb) in enumerate(zip(enc, pbs, cenc, cpbs)):
        assert same_record(r, cr), i
        assert pb == cpb, i
        assert int(r["flags"]) & PATH_BITS == want_bits[i], i
    for (_, _, el), at, kind in zip(split, (0, 4, 7), ("double", "int32", "bool")):
        if at < n:
            assert pbs[at] == wp.record(kind, el)
