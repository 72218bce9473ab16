"""Driver-contract test for bench.py.

The round-end driver launches `python bench.py --gpus N --steps K
--warmup W` and parses ONE JSON line from rank 0; these keys are a hard
interface.  Runs the CPU config (no GPU needed) with a tiny step count."""

import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--config", "cpu",
         "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=300, cwd=str(REPO))
    assert out.returncode == 0, out.stderr[-800:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, key
    assert d["n_gpus"] == 1
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert isinstance(d["value"], (int, float)) and d["value"] > 0
    assert isinstance(d["ms_per_step"], (int, float)) and d["ms_per_step"] > 0
    cfg = d["config"]
    for key in ("model", "global_batch", "seq_len", "parallelism",
                "sessions", "payload_bytes"):
        assert key in cfg, key
    assert cfg["parallelism"] == "dp1"


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last step's response bodies as float .npy
    arrays that decode back to well-formed responses; --full is accepted
    and leaves the result line's contract intact."""
    import numpy as np

    dump = tmp_path / "dump"
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--config", "cpu",
         "--steps", "2", "--warmup", "1", "--batch", "8", "--full",
         "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=300, cwd=str(REPO))
    assert out.returncode == 0, out.stderr[-800:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert sorted(p.name for p in dump.iterdir()) == [
        "response_lengths.npy", "response_rows.npy", "responses.npy"]
    resp = np.load(dump / "responses.npy")
    rows = np.load(dump / "response_rows.npy")
    lens = np.load(dump / "response_lengths.npy")
    assert resp.dtype == np.float32
    assert rows.dtype == lens.dtype == np.float64
    assert rows.tolist() == list(range(8)) and lens.shape == (8,)
    assert resp.shape == (8, int(lens.max()))
    for k in range(8):
        n = int(lens[k])
        assert (resp[k, n:] == -1).all()
        body = json.loads(resp[k, :n].astype(np.uint8).tobytes())
        assert body["id"] == k + 1
        assert body["result"]["isError"] is False
        inner = json.loads(body["result"]["content"][0]["text"])
        assert inner["message"].startswith("Hello, ")


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """Outputs over the size budget keep a fixed, seeded sample of whole
    rows; the lengths of all rows are still recorded."""
    import numpy as np

    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 64)
    responses = [bytes([i]) * (1 + i % 16) for i in range(40)]
    bench.dump_outputs(str(tmp_path / "a"), responses)
    bench.dump_outputs(str(tmp_path / "b"), responses)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy")
         for n in ("responses", "response_rows", "response_lengths")}
    for n, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{n}.npy")), n
    assert a["responses"].shape == (4, 16)
    assert a["response_lengths"].tolist() == [1 + i % 16 for i in range(40)]
    rows = a["response_rows"].astype(int).tolist()
    assert rows == sorted(set(rows)) and all(0 <= r < 40 for r in rows)
    for k, i in enumerate(rows):
        n = 1 + i % 16
        assert (a["responses"][k, :n] == i).all()
        assert (a["responses"][k, n:] == -1).all()
