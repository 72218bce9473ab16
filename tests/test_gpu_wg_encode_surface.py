"""The three corpora through k_json2pb_wg, judged by the oracle.

Every ACCEPT and REJECT case of protojson_corpus, any_corpus and
wide_schema_corpus becomes the ``arguments`` of a tools/call for its schema's
tool, in four textual variants:

* as written (GGRMCP_WG_ENC_MIN=1: the serial scanner, nothing chunks);
* with a ~4 KB pad member spliced in first, and last: a non-packable repeated
  field or a map, so the scanner cuts it into chunk items (kinds 3 and 2)
  while the arguments stay under 8192 bytes;
* with a ~10 KB pad, which takes the arguments to the multi-wave scanner
  (GGRMCP_MW_SCAN=1) or keeps the serial one (=0).

For each variant the oracle parses the same text (the corpora's own verdict
code), the result must equal the classic kernel's (threshold 10^9) in status,
err_pos, aux, id_len and wire bytes, and the path tag in SlotResult.flags
must fit: SR_WG_ITEMS on every status-0 slot unless ``scanner_rule`` names
why the scanner handed the request to the in-block classic pass
(SR_WG_CLASSIC); neither bit at the 10^9 threshold.  One launch per list and
variant.
"""

import json
import os
import re
from contextlib import contextmanager

import pytest

import any_corpus as ac
import protojson_corpus as pc
import wide_schema_corpus as wc
from ggrmcp_amd.engine.batch import SR_WG_CLASSIC, SR_WG_ITEMS

pytestmark = pytest.mark.gpu

WG_ENC_ITEM_PAD = 160     # common.h
WG_ENC_MAX_ITEMS = 384    # common.h
MW_D2 = 512               # json2pb.hip, phase A'


def _gpu(infos):
    from ggrmcp_amd.engine.batch import GpuEngine

    return GpuEngine(infos, device=0)


class Suite:
    """One corpus: its cases, and per case the tool, the message descriptor,
    the pads that fit its schema and the corpus' own verdict code."""

    def __init__(self, name, env, cases, tool_of, desc_of, pads_of, verdicts):
        self.name, self.env, self.cases = name, env, cases
        self.tool_of, self.desc_of, self.pads_of = tool_of, desc_of, pads_of
        self.verdicts = verdicts


def _b64ish(n):
    return "QUJD" * (n // 4)


# pads: (member name, ~4 KB value, ~10 KB value) candidates per schema; the
# first one the case does not name itself is used
_LEAVES = lambda n, w: {f"k{j:03d}": {"id": j, "tag": "t" * w} for j in range(n)}  # noqa: E731
SINK_PADS = [
    ("rBytes", [_b64ish(100)] * 40, [_b64ish(100)] * 100),
    ("mMsg", _LEAVES(50, 60), _LEAVES(120, 60)),
]
ANY_PADS = [
    ("ra", [dict(ac.LEAF, tag="p" * 40)] * 40, [dict(ac.LEAF, tag="p" * 40)] * 100),
    ("ma", {f"k{j:03d}": dict(ac.LEAF, tag="q" * 40) for j in range(40)},
     {f"k{j:03d}": dict(ac.LEAF, tag="q" * 40) for j in range(100)}),
]
WIDE_PADS = {
    "w.Wide": [("f074", ["s" * 100] * 40, ["s" * 100] * 100),
               ("f075", {f"k{j:04d}": j for j in range(350)},
                {f"k{j:04d}": j for j in range(850)})],
    "w.Oneofs": [],       # no repeated or map field: as written only
    "w.Sparse": [("s6", [{"id": j, "tag": "t" * 70} for j in range(45)],
                  [{"id": j, "tag": "t" * 70} for j in range(110)]),
                 ("s3", {f"k{j:04d}": j for j in range(350)},
                  {f"k{j:04d}": j for j in range(850)})],
}


for _name, _small, _big in SINK_PADS + ANY_PADS + sum(WIDE_PADS.values(), []):
    # chunking starts at 2048 bytes; the small pad leaves room under 8192
    assert 2048 + 1024 <= len(json.dumps(_small)) <= 6000, _name
    assert len(json.dumps(_big)) >= 8192 + 1024, _name


def _proto_name(desc, json_name):
    return next(f.name for f in desc.fields if f.json_name == json_name)


def _pick_pad(pads, desc, text):
    for name, small, big in pads:
        if f'"{name}"' not in text and f'"{_proto_name(desc, name)}"' not in text:
            return name, small, big
    return None


def _splice(text, member, first):
    """``member`` as the first or last member of the object ``text``; None if
    the text is not an object from its first to its last byte."""
    if not (text.startswith("{") and text.endswith("}")):
        return None
    body = text[1:-1]
    if not body.strip():
        return "{" + member + "}"
    return "{" + member + "," + body + "}" if first else "{" + body + "," + member + "}"


@pytest.fixture(scope="module")
def suites():
    penv, aenv, wenv = pc.make_env(_gpu), ac.make_env(_gpu), wc.make_env(_gpu)
    sink = penv.sink_cls.DESCRIPTOR
    return [
        Suite("protojson", penv, pc.ACCEPT + pc.REJECT,
              lambda c: penv.sink_tool, lambda c: sink, lambda c: SINK_PADS,
              lambda cs, enc, pbs: pc.encode_verdicts(
                  cs, [penv.sink_cls] * len(cs), enc, pbs)),
        Suite("any", aenv, ac.ACCEPT + ac.REJECT,
              lambda c: aenv.tool, lambda c: aenv.cls.DESCRIPTOR,
              lambda c: ANY_PADS,
              lambda cs, enc, pbs: ac.encode_verdicts(aenv, cs, enc, pbs)),
        Suite("wide", wenv, wc.ACCEPT + wc.REJECT,
              lambda c: wenv.tool[c.msg], lambda c: wenv.cls[c.msg].DESCRIPTOR,
              lambda c: WIDE_PADS[c.msg],
              lambda cs, enc, pbs: pc.encode_verdicts(
                  cs, [wenv.cls[c.msg] for c in cs], enc, pbs)),
    ]


def variant_cases(suite, variant):
    """The suite's cases with the variant's pad spliced in; cases the pad
    does not fit (not an object, or no pad field left) are left out."""
    if variant == "plain":
        return list(suite.cases)
    out = []
    for c in suite.cases:
        pad = _pick_pad(suite.pads_of(c), suite.desc_of(c), c.data)
        if pad is None:
            continue
        name, small, big = pad
        value = big if variant.startswith("big") else small
        text = _splice(c.data, f"{json.dumps(name)}:{json.dumps(value)}",
                       first=variant != "small-last")
        if text is not None:
            out.append(c._replace(data=text))
    return out


# ---- the scanner's rules, from the text alone ---------------------------------

_STR = re.compile(r'"(?:[^"\\]|\\.)*"')
_WS = " \t\r\n"


def top_members(text):
    """[(raw key text without quotes, value start, value end)] of the object
    ``text``, or None if it is not well-formed that far."""
    dec = json.JSONDecoder()
    i, n, out = 0, len(text), []

    def ws(i):
        while i < n and text[i] in _WS:
            i += 1
        return i

    i = ws(i)
    if i >= n or text[i] != "{":
        return None
    i = ws(i + 1)
    if i < n and text[i] == "}":
        return out
    while True:
        m = _STR.match(text, ws(i))
        if not m:
            return None
        i = ws(m.end())
        if i >= n or text[i] != ":":
            return None
        i = ws(i + 1)
        try:
            _, j = dec.raw_decode(text, i)
        except ValueError:
            return None
        out.append((m.group()[1:-1], m.start(), j))
        i = ws(j)
        if i < n and text[i] == ",":
            i += 1
            continue
        return out if i < n and text[i] == "}" else None


def comma_counts(text):
    """Commas directly inside the object ``text`` and one level further in."""
    depth, in_str, esc, n1, n2 = 0, False, False, 0, 0
    for ch in text:
        if in_str:
            if esc:
                esc = False
            elif ch == "\\":
                esc = True
            elif ch == '"':
                in_str = False
        elif ch == '"':
            in_str = True
        elif ch in "{[":
            depth += 1
        elif ch in "}]":
            depth -= 1
        elif ch == ",":
            n1 += depth == 1
            n2 += depth == 2
    return n1, n2


def scanner_rule(desc, text, pb_cap, mw):
    """Why k_json2pb_wg's scanner hands ``text`` (the arguments object of a
    message ``desc``) to the in-block classic pass, or None.  The rules of
    the kernel's header comment: an escaped top-level key, an unknown or
    duplicate top-level member (a second member of one oneof included), the
    index limits of ``seen_mark``, and the item scratch cap (every item gets
    span + span/4 + WG_ENC_ITEM_PAD bytes of a scratch twice the slot's pb
    span, so many small members in a small request do not fit).  ``mw``: the
    multi-wave scanner is on; it takes arguments of 8192 bytes or more and
    collects at most WG_ENC_MAX_ITEMS members and MW_D2 commas one level
    down."""
    members = top_members(text)
    if members is None:
        return "malformed"
    if mw and len(text) >= 8192:
        n1, n2 = comma_counts(text)
        if n1 + 1 > WG_ENC_MAX_ITEMS or n2 > MW_D2:
            return "multi-wave comma cap"
    fields = sorted(desc.fields, key=lambda f: f.number)
    by_name = {}
    for k, f in enumerate(fields):
        by_name[f.name] = by_name[f.json_name] = (k, f)
    seen, oneofs, need = set(), set(), 0
    for key, start, end in members:
        if "\\" in key:
            return "escaped top-level key"
        if key not in by_name:
            return "unknown top-level member"
        k, f = by_name[key]
        real_oneof = f.containing_oneof is not None and not (
            len(f.containing_oneof.fields) == 1
            and f.containing_oneof.name == "_" + f.name)
        if k >= 128 or (real_oneof and f.containing_oneof.index >= 64):
            return "index limit"
        if k in seen or (real_oneof and f.containing_oneof.index in oneofs):
            return "duplicate top-level member"
        seen.add(k)
        if real_oneof:
            oneofs.add(f.containing_oneof.index)
        span = end - start
        chunks = 1 + span // 4096 if span >= 2048 else 1
        need += span + span // 4 + WG_ENC_ITEM_PAD * (chunks + 1)
    if need > 2 * pb_cap:
        return "item scratch cap"
    return None


# ---- runs ---------------------------------------------------------------------

@contextmanager
def _setenv(**kw):
    os.environ.update(kw)
    try:
        yield
    finally:
        for k in kw:
            os.environ.pop(k, None)


VARIANTS = {
    "plain": {},
    "small-first": {},
    "small-last": {},
    "big-mw": {"GGRMCP_MW_SCAN": "1"},
    "big-serial": {"GGRMCP_MW_SCAN": "0"},
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("which", [0, 1, 2], ids=["protojson", "any", "wide"])
def test_wg_encode_corpus(suites, which, variant):
    s = suites[which]
    cases = variant_cases(s, variant)
    assert cases
    bodies = [wc.envelope(s.tool_of(c), c.data, i) for i, c in enumerate(cases)]
    if variant.startswith("big"):
        assert min(len(c.data) for c in cases) >= 8192
    with _setenv(GGRMCP_WG_ENC_MIN="1", **VARIANTS[variant]):
        enc, pbs = s.env.engine.encode_batch(bodies, mode=0, enforce=False)
    with _setenv(GGRMCP_WG_ENC_MIN="1000000000"):
        cenc, cpbs = s.env.engine.encode_batch(bodies, mode=0, enforce=False)
    bad = {k: v for k, v in s.verdicts(cases, enc, pbs).items() if v}
    for c, b, r, cr, pb, cpb in zip(cases, bodies, enc, cenc, pbs, cpbs):
        why = []
        for key in ("status", "err_pos", "aux", "id_len"):
            if int(r[key]) != int(cr[key]):
                why.append(f"{key} {int(r[key])} != classic {int(cr[key])}")
        if (None if pb is None else bytes(pb)) != \
                (None if cpb is None else bytes(cpb)):
            why.append("wire differs from the classic kernel's")
        flags, cflags = int(r["flags"]), int(cr["flags"])
        if cflags & (SR_WG_ITEMS | SR_WG_CLASSIC):
            why.append(f"classic kernel set a path bit ({cflags})")
        if bool(flags & SR_WG_ITEMS) == bool(flags & SR_WG_CLASSIC):
            why.append(f"exactly one path bit expected (flags {flags})")
        if int(r["status"]) == 0 and flags & SR_WG_CLASSIC:
            pb_cap = (len(b) + len(b) // 4 + 192 + 15) & ~15
            rule = scanner_rule(s.desc_of(c), c.data, pb_cap,
                                mw=VARIANTS[variant].get("GGRMCP_MW_SCAN") != "0")
            if rule is None:
                why.append("status 0 from the in-block classic pass, and no "
                           "scanner rule applies")
        if why:
            bad[c.id] = "; ".join(why) + (" | " + bad[c.id] if c.id in bad else "")
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())
