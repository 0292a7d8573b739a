"""bench.py's plain run and --dump-outputs.  CPU: the writer (names, float32, the 64 MB cap).  GPU: one short plain run --
the headline fields, exactly --steps timed steps, none of the --full measurements -- and the scores it dumped equal the
timed path on the same seeded inputs computed in a separate process."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
DEV = "cuda:0"


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=540)


def test_dump_outputs_writes_float32_npy(tmp_path):
    import bench
    s = torch.arange(10, dtype=torch.float64).reshape(2, 5, 1)
    bench.dump_outputs(str(tmp_path / "d"), {"scores": s})
    bench.dump_outputs(str(tmp_path / "d"), {"scores": s + 1}, rank=1)
    assert sorted(os.listdir(tmp_path / "d")) == ["scores.npy", "scores_rank1.npy"]
    got = np.load(tmp_path / "d" / "scores.npy")
    assert got.dtype == np.float32 and got.shape == (2, 5, 1) and np.array_equal(got, s.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "d" / "scores_rank1.npy"), got + 1)
    with pytest.raises(AssertionError, match="64 MB"):
        bench.dump_outputs(str(tmp_path / "big"), {"x": torch.zeros((64 << 20) // 4 + 1)})


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_line_and_dumped_scores(tmp_path):
    p = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "impressions/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    # value and ms_per_step describe the same timed steps: B impressions per step
    assert out["ms_per_step"] > 0 and abs(out["value"] - 512 * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]
    assert "roofline" not in out and "extra" not in out and out["cpu_baseline"] is None
    got = np.load(tmp_path / "scores.npy")
    assert got.dtype == np.float32 and got.shape == (512, 5, 1)

    # the same step on the same seeded inputs, in a child process of its own: this test leaves no model, caches or
    # device memory behind in the test process
    code = textwrap.dedent(f"""
        import bench
        import numpy as np
        import torch
        from xnrs_amd import hip
        dev = torch.device({DEV!r})
        hip.set_gemm_mode(0)
        model, _ = bench.build_model(bench.WORKLOAD, dev)
        hist, cand = bench.make_inputs(bench.WORKLOAD, dev, seed=1000)
        with torch.no_grad():
            np.save({str(tmp_path / "want.npy")!r}, bench.step(model, hist, cand).cpu().numpy())
    """)
    q = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert q.returncode == 0, q.stderr[-3000:]
    assert np.array_equal(got, np.load(tmp_path / "want.npy"))
