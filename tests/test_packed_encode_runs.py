"""Packed numeric arrays on encode, CPU build (WAVE=1: a window is one
element): the lane parser and the integer-only decimal-to-binary converter
(csrc/fp_parse.h) against ``float(text)`` / ``int(text)`` packed with
``struct``, byte for byte.  ``test_gpu_packed_encode_runs.py`` runs the same
lists through the 64-lane windows."""

import pytest

import packed_encode_corpus as pe
import protojson_corpus as pc


@pytest.fixture(scope="module")
def env():
    from ggrmcp_amd.engine.hostsim import HostSimEngine

    return pc.make_env(HostSimEngine)


def test_host_rules_gone_inside_packed_arrays(env):
    """Fails on the parent (E_UNSUPPORTED): near-denormal, near-DBL_MAX and
    long-mantissa doubles, as written and quoted; the dropped-digits tie
    stays with the host."""
    cases = [c for c in pc.ACCEPT if c.id in pe.HOST_RULE_CASES]
    assert len(cases) == 3
    arrays = [pe.doc_texts(c.data) for c in cases] + [pe.EXTREMES_65]
    pe.check_exact(env, "double", arrays + [pe.quoted(a) for a in arrays])
    plain = [c._replace(host=None) for c in cases]
    assert not {k: v for k, v in pc.run_encode(env, plain).items() if v}
    assert pe.encode(env, [pe.TIE_DOC])[0][0] == pe.E_UNSUPPORTED


@pytest.mark.parametrize("kind,texts", [("double", pe.DOUBLE_TEXTS),
                                        ("float", pe.FLOAT_TEXTS)])
def test_every_binary_exponent(env, kind, texts):
    pe.check_exact(env, kind, [texts[i:i + 64] for i in range(0, len(texts), 64)])


@pytest.mark.parametrize("kind", pe.KINDS)
def test_window_geometry(env, kind):
    pe.check_exact(env, kind, [pe.doc_texts(d) for d in pe.geometry_docs(kind)])


@pytest.mark.parametrize("at", pe.ODD_AT)
def test_declined_pieces_keep_the_serial_answer(env, at):
    ok = [pe.odd_doc(o, at) for o in pe.ODD_OK]
    for d, (status, _, _, wire) in zip(ok, pe.encode(env, ok)):
        assert status == 0 and wire == pe.ref_wire("int32", pe.doc_texts(d))
    bad = [pe.odd_doc(o, at) for o, _ in pe.ODD_BAD] + [pe.odd_doc(str(at), at, "")]
    want = [s for _, s in pe.ODD_BAD] + [pe.E_PARSE]
    for d, w, (status, err_pos, _, _) in zip(bad, want, pe.encode(env, bad)):
        assert status == w, d[:40]
        # the serial element's own position: at or after the odd element
        assert err_pos >= len('{"rInt32":[') + sum(len(str(i)) + 1 for i in range(at))


def test_overflow_is_the_serial_paths(env):
    assert pe.encode(env, [pe.OVERFLOW_DOC])[0][0] == pe.E_OVERFLOW
