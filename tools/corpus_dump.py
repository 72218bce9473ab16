"""Write the protojson corpus (tests/protojson_corpus.py), the Any corpus
(tests/any_corpus.py) and their compiled tables to one binary file for
tools/asan_corpus.cpp — the stand-alone sanitizer run of the kernel logic
(no Python in the sanitized process).

The file is a sequence of sections, one per schema, until end of file.
Section layout (little endian): 7 table blobs (CompiledTables.blobs(), the
type table last), each u32 length + bytes; i32 n_msgs, i32 n_tools; u32 case
count; per case: u8 direction (0 = JSON -> pb, 1 = pb -> JSON), i32 message
index, u32 length, bytes.
"""

import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import any_corpus as ac  # noqa: E402
import protojson_corpus as pc  # noqa: E402
from ggrmcp_amd.engine.tables import compile_tables  # noqa: E402


class _Tables:
    def __init__(self, infos):
        self.tables = compile_tables(infos)


def _write_section(f, t, cases) -> None:
    blobs = t.blobs()
    assert len(blobs) == 7
    for blob in blobs:
        f.write(struct.pack("<I", len(blob)) + blob)
    f.write(struct.pack("<iiI", t.n_msgs, t.n_tools, len(cases)))
    for d, idx, data in cases:
        f.write(struct.pack("<BiI", d, idx, len(data)) + data)


def _any_cases(env):
    cases = []
    for c in ac.ACCEPT + ac.REJECT + ac.ORACLE_DECIDES:
        cases.append((0, env.idx, c.data.encode()))
    for w in ac.accept_wires(env) + [c.data for c in ac.WIRES]:
        cases.append((1, env.idx, w))
    # every prefix of the richest payloads: truncation at each byte
    text = next(c for c in ac.ACCEPT if c.id == "all-fields").data.encode()
    wire = next(w for c, w in zip(ac.ACCEPT, ac.accept_wires(env))
                if c.id == "all-fields")
    cases += [(0, env.idx, text[:k]) for k in range(len(text))]
    cases += [(1, env.idx, wire[:k]) for k in range(len(wire))]
    return cases


def main(out_path: str) -> None:
    env = pc.make_env(_Tables)
    t = env.engine.tables
    cases = []
    for c in pc.ACCEPT + pc.REJECT + pc.PY_LAX + pc.GO_STRICT:
        cases.append((0, env.sink_idx, c.data.encode()))
    for w in pc.accept_wires(env) + [c.data for c in pc.WIRES]:
        cases.append((1, env.sink_idx, w))
    for b in pc.utf8_cases():
        cases.append((0, env.inner_idx, b'{"key":"' + b + b'"}'))
        cases.append((1, env.inner_idx, pc.ld(1, b)))
    for b in pc.whitespace_cases():
        cases.append((0, env.inner_idx, b))
    any_env = ac.make_env(_Tables)
    any_cases = _any_cases(any_env)
    with open(out_path, "wb") as f:
        _write_section(f, t, cases)
        _write_section(f, any_env.engine.tables, any_cases)
    print(f"{len(cases)} + {len(any_cases)} Any cases -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1])
