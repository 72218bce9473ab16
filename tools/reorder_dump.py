"""Write the DM_REORDER cases and their compiled tables to one binary file for
tools/asan_reorder.cpp — the stand-alone sanitizer run of k_pb_reorder's
phases (no Python in the sanitized process).

Cases: every wire of tests/reorder_corpus.py as kinds 0, 1, 2 and with
DM_UNPOPULATED | DM_STRUCTURED, and every byte-prefix of the richest x.Rich
wire (the repeated, merged-message, oneof, map and unknown-field cases
concatenated: a concatenation is itself a wire), as bare JSON.

File layout: that of tools/structured_dump.py (see tools/wg_decode_dump.py).
"""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

import reorder_corpus as rc  # noqa: E402
import unpopulated_corpus as uc  # noqa: E402
from structured_dump import _Tables, _write_section  # noqa: E402

RO = rc.DM_REORDER
MODES = (0 | RO, 1 | RO, 2 | RO, 0 | RO | uc.DM_UNPOPULATED | uc.DM_STRUCTURED)


def main(out_path: str) -> None:
    envs = rc.make_envs(_Tables)
    sections = {}
    for name, wire, _ in rc.CASES.values():
        s = envs.schema(name)
        sections.setdefault(id(s.engine), (s.engine.tables, []))[1].extend(
            (m, s.idx, b"7", wire) for m in MODES)
    rich = b"".join(rc.CASES[c][1] for c in (
        "repeated-scalar-3-runs", "repeated-message-split", "message-merge",
        "oneof-X1-Y-X2", "map-split", "unknowns", "swap-in-map-value"))
    s = envs.schema("x.Rich")
    sections[id(s.engine)][1].extend(
        (1 | RO, s.idx, b"7", rich[:k]) for k in range(len(rich) + 1))
    with open(out_path, "wb") as f:
        for tables, cases in sections.values():
            _write_section(f, tables, cases)
    print(" + ".join(str(len(c)) for _, c in sections.values()), "cases ->", out_path)


if __name__ == "__main__":
    main(sys.argv[1])
