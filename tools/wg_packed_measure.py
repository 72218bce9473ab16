"""Workload behind profiles/wg_packed_chunks.md: envelope decode batches of 64
slots through ``k_pb2json_wg``, to be run under ``rocprofv3 --kernel-trace``.

In order: one top-level packed run per slot of 16 KB and of 64 KB, as
``double``, ``float``, ``int32`` (one-byte elements) and ``int64`` (ten-byte
elements); then bench.Wide64 responses of 64 KB, which hold no packed run.
Every shape is decoded WARM + REPS times, so the kernel's dispatches in the
trace map to shapes by their order.  ``--so DIR`` loads the device extension
from DIR instead of the tree's, to time another build of it.
"""

import argparse
import importlib.util
import json
import random
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
WARM, REPS, SLOTS = 2, 5, 64


def body(kind: str, nbytes: int) -> bytes:
    from protojson_corpus import vi

    if kind in ("double", "float"):
        fmt, w = ("<d", 8) if kind == "double" else ("<f", 4)
        return b"".join(struct.pack(fmt, i * 0.37 + 0.001) for i in range(nbytes // w))
    if kind == "int32":
        return bytes(i % 100 for i in range(nbytes))
    return vi(2**64 - 1) * -(-nbytes // 10)  # int64 -1


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--so", help="directory of another _jsonproto.so")
    args = ap.parse_args()
    import ggrmcp_amd.ops as ops
    if args.so:
        name = "ggrmcp_amd.ops._jsonproto"
        spec = importlib.util.spec_from_file_location(name, Path(args.so) / "_jsonproto.so")
        sys.modules[name] = ops._jsonproto = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ops._jsonproto)

    import packed_chunk_cases as cc
    import packed_runs_corpus as pr
    import protojson_corpus as pc
    from google.protobuf import json_format

    from ggrmcp_amd.engine.batch import GpuEngine
    from ggrmcp_amd.utils.synthetic import wide_payload

    def gpu(infos):
        return GpuEngine(infos, device=0)

    holders, env = cc.make_holders(gpu), pc.make_env(gpu)
    shapes = [(holders[cc.FIELD[k][0]], pc.ld(cc.FIELD[k][1], body(k, size)))
              for k in ("double", "float", "int32", "int64") for size in (16384, 65536)]
    wide = json_format.ParseDict(wide_payload(random.Random(7), target_bytes=65536),
                                 env.wide_cls()).SerializeToString()
    assert len(wide) >= 16384
    shapes.append(((env.engine, env.wide_cls, env.wide_idx, env.sink_tool), wide))
    ok = True
    for (engine, _, idx, tool), wire in shapes:
        bodies = [json.dumps({"jsonrpc": "2.0", "id": i, "method": "tools/call",
                              "params": {"name": tool, "arguments": {}}}).encode()
                  for i in range(SLOTS)]
        for _ in range(WARM + REPS):
            engine.encode_batch(bodies, mode=0)
            dec, _ = engine.decode_batch([wire] * SLOTS, [idx] * SLOTS, mode=0)
            ok &= all(int(r["status"]) == 0 and int(r["pad"]) == 1 for r in dec)
    print("wg_packed_measure:", "ok" if ok else "a slot was not answered by the item walk")
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
