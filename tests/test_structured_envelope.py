"""The structured result envelope of k_pb2json (mode 0 with DM_UNPOPULATED |
DM_STRUCTURED) on the CPU build:

  {"jsonrpc":"2.0","id":<id>,"result":{"content":[{"type":"text","text":
  "<escaped>"}],"structuredContent":<raw>,"isError":false}}

and that nothing else moved: mode 2 ignores the flags, modes 0 and 1 without
flags still print what the protojson oracle prints."""

import json

import pytest

import protojson_corpus as pc
import unpopulated_corpus as uc
from ggrmcp_amd.engine.cpu_ref import CpuTranscoder
from ggrmcp_amd.engine.hostsim import HostSimEngine

FLAGS = uc.DM_UNPOPULATED | uc.DM_STRUCTURED


@pytest.fixture(scope="module")
def envs():
    return uc.make_envs(HostSimEngine)


@pytest.fixture(scope="module")
def sweep(envs):
    """Every sweep string as bench.Inner.key, ids cycling through numeric,
    string, null and 48-byte tokens."""
    env = envs.sink
    s = envs.schema("bench.Inner")
    strings = uc.envelope_strings()
    wires = [env.inner_cls(key=t).SerializeToString() for t in strings]
    ids = [uc.ENV_IDS[i % len(uc.ENV_IDS)] for i in range(len(wires))]
    outs = uc.run_envelopes(s, env.sink_tool, wires, ids, FLAGS)
    return strings, ids, outs


def test_sweep_covers_the_cases():
    strings = uc.envelope_strings()
    assert {len(t) for t in strings} == set(uc.ENV_LENGTHS)
    assert len(uc.id_token(uc.ENV_IDS[-1])) == 48
    assert len(strings) == 1 + 6 * (2 * len(uc.ENV_LENGTHS[1:]))


@pytest.mark.parametrize("k", range(len(uc.envelope_strings())))
def test_envelope(sweep, k):
    strings, ids, outs = sweep
    status, out = outs[k]
    assert status == 0, status
    why = uc.check_envelope(out, uc.id_token(ids[k]))
    assert why is None, why
    sc = json.loads(out)["result"]["structuredContent"]
    # bench.Inner: key, value (int64), weight (double) — all without presence
    assert sc == {"key": strings[k], "value": "0", "weight": 0}


def test_empty_reply_satisfies_required(envs):
    s = envs.schema("hello.HelloResponse")
    tool = next(n for n, mi in envs.infos.items()
                if mi.output_descriptor.full_name == "hello.HelloResponse")
    (status, out), = uc.run_envelopes(s, tool, [b""], [1], FLAGS)
    assert status == 0
    assert out == (b'{"jsonrpc":"2.0","id":1,"result":{"content":[{"type":"text",'
                   b'"text":"{\\"message\\":\\"\\"}"}],"structuredContent":'
                   b'{"message":""},"isError":false}}')


def test_skipped_and_failing_slots(envs):
    """A skipped slot stays empty and a failing wire keeps its status; their
    neighbours are unaffected."""
    env = envs.sink
    s = envs.schema("bench.Inner")
    good = env.inner_cls(key="k", value=3).SerializeToString()
    wires = [good, None, pc.ld(1, b"bad\x80"), good]
    outs = uc.run_envelopes(s, env.sink_tool, wires, [0, 1, 2, 3], FLAGS)
    assert [st for st, _ in outs] == [0, 0, pc.E_UNSUPPORTED, 0]
    assert outs[1][1] is None and outs[2][1] is None
    for k in (0, 3):
        assert uc.check_envelope(outs[k][1], uc.id_token(k)) is None


def test_streaming_item_ignores_the_flags(envs):
    env = envs.sink
    s = envs.schema("bench.Inner")
    wires = [b"", env.inner_cls(key='q"').SerializeToString(),
             env.inner_cls(value=5).SerializeToString()]
    idx = [s.idx] * len(wires)
    _, plain = s.engine.decode_batch(wires, idx, mode=2)
    _, flagged = s.engine.decode_batch(wires, idx, mode=2 | FLAGS)
    assert plain == flagged
    assert plain[0] == b'{"type":"text","text":"{}"}'


def _dozen(envs):
    env = envs.sink
    ids = ["int-ext-num-int64", "dbl-plain", "flt-plain", "enum-list", "b64-list",
           "map-key-string", "map-val-msg", "dur-list", "val-nested",
           "wrappers-values", "optional-zero", "leaf"]
    by_id = dict(zip((c.id for c in pc.ACCEPT), pc.accept_wires(env)))
    return [by_id[i] for i in ids]


@pytest.mark.parametrize("mode", [0, 1])
def test_modes_without_flags_unchanged(envs, mode):
    """Modes 0 and 1 with no flag: a dozen corpus wires still print what
    cpu_ref (protojson, default omission) prints, inside today's envelope."""
    env = envs.sink
    s = envs.schema("t.Sink")
    wires = _dozen(envs)
    cpu = CpuTranscoder()
    desc = env.sink_cls.DESCRIPTOR
    if mode == 0:
        outs = uc.run_envelopes(s, env.sink_tool, wires, list(range(len(wires))), 0)
    else:
        outs = uc.decode(s, wires, 0)
    for i, (w, (status, out)) in enumerate(zip(wires, outs)):
        assert status == 0
        want = pc.loads(cpu.pb_to_json(desc, w))
        if mode == 0:
            resp = json.loads(out)
            assert list(resp["result"]) == ["content", "isError"]
            assert b"structuredContent" not in out
            assert resp["id"] == i
            text = resp["result"]["content"][0]["text"]
        else:
            text = out.decode()
        assert pc.same_json(pc.loads(text), want, desc), (text, want)


def test_cpu_ref_option_matches_kernel(envs):
    """cpu_ref's new option is the same printer the kernel is judged by."""
    s = envs.schema("x.Rich")
    cpu = CpuTranscoder()
    desc = s.cls.DESCRIPTOR
    assert json.loads(cpu.pb_to_json(desc, b"")) == {}
    full = json.loads(cpu.pb_to_json(desc, b"", unpopulated=True))
    (status, out), = uc.decode(s, [b""], uc.DM_UNPOPULATED)
    assert status == 0 and json.loads(out) == full and "sEnum" in full
