"""Packed numeric arrays on encode, gfx950: the 64-lane windows of
``pk_window`` (csrc/fp_parse.h: separator masks, rank-select, per-lane parse,
prefix commit, scan of varint lengths, stores) against ``float(text)`` /
``int(text)`` byte for byte, and against the CPU build's result record where
the window declines."""

import os

import pytest

import packed_encode_corpus as pe
import protojson_corpus as pc
import wide_schema_corpus as wc
from ggrmcp_amd.engine.batch import SR_WG_CLASSIC, SR_WG_ITEMS

pytestmark = pytest.mark.gpu


def _gpu(infos):
    from ggrmcp_amd.engine.batch import GpuEngine

    return GpuEngine(infos, device=0)


def _cpu(infos):
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return HostSimEngine(infos)


@pytest.fixture(scope="module")
def envs():
    return pc.make_env(_gpu), pc.make_env(_cpu)


def test_host_rules_gone_inside_packed_arrays(envs):
    gpu, _ = envs
    arrays = [pe.doc_texts(c.data) for c in pc.ACCEPT
              if c.id in pe.HOST_RULE_CASES] + [pe.EXTREMES_65]
    assert len(arrays) == 4
    pe.check_exact(gpu, "double", arrays + [pe.quoted(a) for a in arrays])
    assert pe.encode(gpu, [pe.TIE_DOC])[0][0] == pe.E_UNSUPPORTED


@pytest.mark.parametrize("kind,texts", [("double", pe.DOUBLE_TEXTS),
                                        ("float", pe.FLOAT_TEXTS)])
def test_every_binary_exponent(envs, kind, texts):
    pe.check_exact(envs[0], kind, [texts[i:i + 64] for i in range(0, len(texts), 64)])


@pytest.mark.parametrize("kind", pe.KINDS)
def test_window_geometry(envs, kind):
    arrays = [pe.doc_texts(d) for d in pe.geometry_docs(kind)]
    for filler in range(4):
        pe.check_exact(envs[0], kind, arrays, filler)


def test_declined_pieces_keep_the_serial_answer(envs):
    """Result record and wire of the CPU build, whose window is one element
    and whose errors are therefore the serial path's."""
    gpu, cpu = envs
    docs = [pe.odd_doc(o, at) for at in pe.ODD_AT
            for o in pe.ODD_OK + [o for o, _ in pe.ODD_BAD]]
    docs += [pe.odd_doc(str(at), at, "") for at in pe.ODD_AT] + [pe.OVERFLOW_DOC]
    got, want = pe.encode(gpu, docs), pe.encode(cpu, docs)
    assert got == want
    assert want[-1][0] == pe.E_OVERFLOW and want[0][0] == 0


def test_workgroup_kernel(envs):
    """One 20 KB request through k_json2pb_wg: the packed array is one
    member item, so one wave's windows; the classic kernel's wire."""
    gpu, _ = envs
    body = wc.envelope(gpu.sink_tool, pe.WG_DOC, 1)
    enc, pbs = gpu.engine.encode_batch([body], mode=0, enforce=False)
    os.environ["GGRMCP_WG_ENC_MIN"] = "1000000000"
    try:
        cenc, cpbs = gpu.engine.encode_batch([body], mode=0, enforce=False)
    finally:
        os.environ.pop("GGRMCP_WG_ENC_MIN", None)
    assert int(enc[0]["status"]) == 0 and int(cenc[0]["status"]) == 0
    assert int(enc[0]["flags"]) & (SR_WG_ITEMS | SR_WG_CLASSIC) == SR_WG_ITEMS
    assert int(cenc[0]["flags"]) & (SR_WG_ITEMS | SR_WG_CLASSIC) == 0
    assert pbs[0] == cpbs[0]
    assert pbs[0].startswith(pe.ref_wire("double", pe.WG_TEXTS))
