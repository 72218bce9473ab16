"""Workload behind profiles/wg_packed_encode.md: tools/call batches of 64 slots
through ``k_json2pb_wg``, to be run under ``rocprofv3 --kernel-trace``.

In order: one packed array per slot whose text is 16 KB and 64 KB long, as
``double``, ``fixed32``, ``int32`` (one-byte elements) and ``bool``.  Every
shape is encoded WARM + REPS times, so the kernel's dispatches in the trace
map to shapes by their order.  ``GGRMCP_MW_SCAN=0`` in the environment selects
the serial scanner.  ``--so DIR`` loads the device extension from DIR instead
of the tree's, to time another build of it.  Prints, per shape, the path bits
of ``SlotResult.flags`` the slots came back with.
"""

import argparse
import importlib.util
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
WARM, REPS, SLOTS = 2, 5, 64
KINDS = ("double", "fixed32", "int32", "bool")
SIZES = (16384, 65536)


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

    import protojson_corpus as pc
    import wg_packed_encode_cases as wp
    import wide_schema_corpus as wc

    from ggrmcp_amd.engine.batch import GpuEngine

    env = pc.make_env(lambda infos: GpuEngine(infos, device=0))
    ok = True
    for kind in KINDS:
        for size in SIZES:
            el = wp.elements(kind, size)
            doc = '{"%s":[%s]}' % (wp.field_name(kind), ",".join(el))
            bodies = [wc.envelope(env.sink_tool, doc, i) for i in range(SLOTS)]
            for _ in range(WARM + REPS):
                enc, pbs = env.engine.encode_batch(bodies, mode=0, enforce=False)
            ok &= all(int(r["status"]) == 0 for r in enc)
            ok &= pbs[0] == wp.record(kind, el) and pbs[-1] == pbs[0]
            print(f"{kind}-{size // 1024}K: {len(el)} elements, path bits "
                  f"{sorted({int(r['flags']) & 28 for r in enc})}")
    print("wg_packed_encode_measure:", "ok" if ok else "a slot failed or differs")
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
