"""Write the DM_UNPOPULATED / DM_STRUCTURED decode cases and their compiled
tables to one binary file for tools/asan_structured.cpp — the stand-alone
sanitizer run of the decode kernel with the new flags (no Python in the
sanitized process).

Cases: both corpora (tests/protojson_corpus.py, tests/any_corpus.py) and the
targeted cases of tests/unpopulated_corpus.py as bare JSON with
DM_UNPOPULATED; the envelope string sweep with both flags and every id
shape; every byte-prefix of the richest wires in both forms.

The file is a sequence of sections, one per table set, until end of file.
Section layout (little endian): 7 table blobs, each u32 length + bytes;
i32 n_msgs, i32 n_tools; u32 case count; per case: u8 decode mode, i32
message index, u32 id length + id token bytes, u32 wire length + bytes.
"""

import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import any_corpus as ac  # noqa: E402
import protojson_corpus as pc  # noqa: E402
import unpopulated_corpus as uc  # noqa: E402
from ggrmcp_amd.engine.tables import compile_tables  # noqa: E402

BARE = 1 | uc.DM_UNPOPULATED
ENVELOPE = 0 | uc.DM_UNPOPULATED | uc.DM_STRUCTURED


class _Tables:
    def __init__(self, infos):
        self.tables = compile_tables(infos)


def _write_section(f, t, cases) -> None:
    blobs = t.blobs()
    assert len(blobs) == 7
    for blob in blobs:
        f.write(struct.pack("<I", len(blob)) + blob)
    f.write(struct.pack("<iiI", t.n_msgs, t.n_tools, len(cases)))
    for mode, idx, rid, data in cases:
        f.write(struct.pack("<BiI", mode, idx, len(rid)) + rid)
        f.write(struct.pack("<I", len(data)) + data)


def _both(idx, wire, rid=b"7"):
    return [(BARE, idx, b"", wire), (ENVELOPE, idx, rid, wire)]


def main(out_path: str) -> None:
    envs = uc.make_envs(_Tables)
    sections = {"sink": [], "holder": [], "third": []}

    def bucket(name):
        if name in ("t.Sink", "bench.Wide64", "bench.Inner"):
            return sections["sink"]
        return sections["holder"] if name == "t.Holder" else sections["third"]

    for name, wire in uc.corpus_wires(envs).values():
        bucket(name).extend(_both(envs.schema(name).idx, wire))
    for name, wire, _ in uc.targeted_cases(uc.sink_descriptor()).values():
        bucket(name).extend(_both(envs.schema(name).idx, wire))
    name, wire = uc.expansion_case()
    bucket(name).extend(_both(envs.schema(name).idx, wire))
    # envelope sweep: every string, every id shape
    inner = envs.schema("bench.Inner")
    for k, text in enumerate(uc.envelope_strings()):
        rid = uc.id_token(uc.ENV_IDS[k % len(uc.ENV_IDS)])
        w = envs.sink.inner_cls(key=text).SerializeToString()
        sections["sink"].append((ENVELOPE, inner.idx, rid, w))
    # every byte-prefix of the richest wires: truncation at each byte
    rich = next(w for c, w in zip(ac.ACCEPT, ac.accept_wires(envs.holder))
                if c.id == "all-fields")
    for k in range(len(rich) + 1):
        sections["holder"].extend(_both(envs.holder.idx, rich[:k]))
    cases = uc.targeted_cases(uc.sink_descriptor())
    third = (cases["zero:all"][1] + pc.ld(21, pc.ld(2, b"t")) + pc.ld(22, b"") * 2
             + pc.ld(23, pc.ld(1, b"k")) + pc.ld(24, pc.ld(1, b"k"))
             + pc.ld(40, b"\x01\x02") + pc.ld(1000, b"z"))
    idx = envs.schema("x.Rich").idx
    for k in range(len(third) + 1):
        sections["third"].extend(_both(idx, third[:k]))
    with open(out_path, "wb") as f:
        _write_section(f, envs.sink.engine.tables, sections["sink"])
        _write_section(f, envs.holder.engine.tables, sections["holder"])
        _write_section(f, envs.engine.tables, sections["third"])
    print(" + ".join(str(len(v)) for v in sections.values()), "cases ->", out_path)


if __name__ == "__main__":
    main(sys.argv[1])
