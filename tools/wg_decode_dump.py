"""Write the workgroup-decode cases and their compiled tables to one binary
file for tools/asan_wg_decode.cpp — the stand-alone sanitizer run of
k_pb2json_wg's host driver (no Python in the sanitized process).

Cases: every group of tests/wg_flags_corpus.py (both corpora, the targeted
cases, sparse bench.Wide64, the chunk joins, the hand-assembled top-level
wires, the top-level Any) and every byte-prefix of the richest x.Rich and
bench.Wide64 wires, each as an envelope with the flags clear, with
DM_UNPOPULATED, and with DM_UNPOPULATED | DM_STRUCTURED.

The file has the layout tools/structured_dump.py writes: a sequence of
sections, one per table set; 7 table blobs, each u32 length + bytes; i32
n_msgs, i32 n_tools; u32 case count; per case: u8 decode mode, i32 message
index, u32 id length + id token bytes, u32 wire length + bytes.
"""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

import protojson_corpus as pc  # noqa: E402
import unpopulated_corpus as uc  # noqa: E402
import wg_flags_corpus as wc  # noqa: E402
from structured_dump import _Tables, _write_section  # noqa: E402


def _modes(idx, wire, rid):
    return [(flags, idx, rid, wire) for flags in wc.FLAG_SETS]


def main(out_path: str) -> None:
    envs = uc.make_envs(_Tables)
    sections = {"sink": [], "holder": [], "third": []}

    def bucket(name):
        if name in ("t.Sink", "bench.Wide64", "bench.Inner"):
            return sections["sink"]
        return sections["holder"] if name == "t.Holder" else sections["third"]

    for k, (name, wire) in enumerate(wc.all_cases(envs).values()):
        rid = uc.id_token(uc.ENV_IDS[k % len(uc.ENV_IDS)])
        bucket(name).extend(_modes(envs.schema(name).idx, wire, rid))
    # every byte-prefix of the richest wires: truncation at each byte
    cases = uc.targeted_cases(uc.sink_descriptor())
    rich = (cases["zero:all"][1] + pc.ld(21, pc.ld(2, b"t")) + pc.ld(22, b"") * 2
            + pc.ld(23, pc.ld(1, b"k")) + pc.ld(24, pc.ld(1, b"k"))
            + pc.ld(40, b"\x01\x02") + pc.ld(1000, b"z"))
    idx = envs.schema("x.Rich").idx
    for k in range(len(rich) + 1):
        sections["third"].extend(_modes(idx, rich[:k], b"7"))
    wide = envs.sink.wide_cls(f01_string='q"\\', f02_int32=-3)
    wide.nested.key = "n"
    for j in range(3):
        wide.items.add(key=f"i{j}\n", value=j, weight=j / 2)
    wide.level = 2
    wide.attrs["a"] = "é"
    wide.attrs["b"] = ""
    wire = wide.SerializeToString()
    idx = envs.schema("bench.Wide64").idx
    for k in range(len(wire) + 1):
        sections["sink"].extend(_modes(idx, wire[:k], b'"w"'))
    with open(out_path, "wb") as f:
        _write_section(f, envs.sink.engine.tables, sections["sink"])
        _write_section(f, envs.holder.engine.tables, sections["holder"])
        _write_section(f, envs.engine.tables, sections["third"])
    print(" + ".join(str(len(v)) for v in sections.values()), "cases ->", out_path)


if __name__ == "__main__":
    main(sys.argv[1])
