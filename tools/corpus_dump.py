"""Write the protojson corpus (tests/protojson_corpus.py) and the compiled
tables to one binary file for tools/asan_corpus.cpp — the stand-alone
sanitizer run of the kernel logic (no Python in the sanitized process).

Layout (little endian): 6 table blobs, each u32 length + bytes; i32 n_msgs,
i32 n_tools; u32 case count; per case: u8 direction (0 = JSON -> pb,
1 = pb -> JSON), i32 message index, u32 length, bytes.
"""

import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import protojson_corpus as pc  # noqa: E402
from ggrmcp_amd.engine.tables import compile_tables  # noqa: E402


class _Tables:
    def __init__(self, infos):
        self.tables = compile_tables(infos)


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
    with open(out_path, "wb") as f:
        for blob in t.blobs():
            f.write(struct.pack("<I", len(blob)) + blob)
        f.write(struct.pack("<iiI", t.n_msgs, t.n_tools, len(cases)))
        for d, idx, data in cases:
            f.write(struct.pack("<BiI", d, idx, len(data)) + data)
    print(f"{len(cases)} cases -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1])
