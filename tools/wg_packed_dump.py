"""Write the packed-chunk cases and their compiled tables to one binary file
for tools/asan_wg_packed.cpp, the stand-alone sanitizer run of the split of
top-level packed runs in k_pb2json_wg's host driver.

Cases: the lists of tests/packed_chunk_cases.py (every kind once, the joined
texts, the malformed runs, the CPU-only runs, the empty run) and every
byte-prefix of one split int64 wire, each as an envelope with the flags
clear, with DM_UNPOPULATED, and with DM_UNPOPULATED | DM_STRUCTURED.  The file
has the layout tools/structured_dump.py writes, one section per schema.
"""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

import packed_chunk_cases as cc  # noqa: E402
from structured_dump import _Tables, _write_section  # noqa: E402

MODES = (0, cc.UNPOP, cc.UNPOP | cc.STRUCT)


def main(out_path: str) -> None:
    holders = cc.make_holders(_Tables)
    wires = [(c[1], c[2]) for c in cc.CASES + cc.CPU_ONLY] + [("c", cc.BATCH[2][0])]
    split = cc.run("int64", *cc.take("int64", cc.BIG + 1))[0]
    wires += [("v", split[:k]) for k in range(len(split) + 1)]
    with open(out_path, "wb") as f:
        for schema, h in holders.items():
            cases = [(m, h[2], b"7", w) for s, w in wires if s == schema for m in MODES]
            _write_section(f, h[0].tables, cases)
            print(schema, len(cases), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
