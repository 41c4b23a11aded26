"""bench.py contract: argument surface on CPU, and on the GPU box the real thing -- a short N=1 run
and the same command under torch.distributed.run with one rank (RCCL init + weight/style broadcast
path of vtoonify_amd/frames.py; multi-GPU boxes are the driver's, the code path is identical)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_to_run_without_gpu_or_with_wrong_world_size():
    env = dict(os.environ, WORLD_SIZE="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def _check(line):
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 1
    assert d["value"] > 30.0, "north-star floor: >= 30 frames/s at 1024x1024 on one MI355X"
    return d


@pytest.mark.gpu
def test_bench_single_process(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "5", "--warmup", "2",
                        "--no-cpu-baseline", "--op-iters", "1", "--no-video", "--min-seconds", "0.2",
                        "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _check(r.stdout.strip().splitlines()[-1])
    # --steps is the timed step count; the last step's frames (4 x 3x1024x1024 float32 = 48 MB) are written whole
    assert d["steps"] == 5 and d["timed_blocks"] == 1
    import numpy as np
    y = np.load(tmp_path / "y.npy")
    assert y.dtype == np.float32 and y.shape == (4, 3, 1024, 1024) and np.isfinite(y).all()
    assert d["n_gpus"] == 1 and d["cpu_baseline"] is None or d["n_gpus"] == 1
    # extra keys: the reference's --batch_size 4, config 3's per-rank step, one frame in flight, and the
    # drop-in module's __call__ (hipGraph by default: within 15 % of the engine's single-stream rate here,
    # short run; the 1-second default run is what DESIGN.md quotes)
    for k in ("batch1", "config3", "single_stream", "module_call"):
        assert d[k]["value"] > 30.0, k
    assert d["config"]["frames_per_step_per_gpu"] == 4
    assert d["timed_blocks"] >= 1 and d["timed_seconds"] > 0
    assert d["module_call"]["value"] > 0.85 * d["single_stream"]["value"], (d["module_call"], d["single_stream"])


@pytest.mark.gpu
def test_bench_under_torch_distributed_run_one_rank():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", "29533", os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--no-cpu-baseline", "--op-iters", "1", "--no-video", "--no-extras", "--min-seconds", "0.1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    _check([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])


def test_bench_dump_outputs_dry_run_emulation(tmp_path):
    """--dump-outputs DIR (host emulation, one process): DIR/y.npy is the float32 copy of what the LAST of exactly
    --steps timed steps returned -- the engine's frames for that step's input (step i runs synthetic frame batch i % 4)
    -- and a second run with the same arguments writes the same bytes."""
    import numpy as np
    import torch
    ys = []
    for run in ("a", "b"):
        out = tmp_path / run
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "3", "--warmup", "1", "--dry-run-emu",
               "--height", "8", "--width", "8", "--lanes", "2", "--dtype", "bf16", "--backbone", "toonify", "--batch", "2",
               "--no-extras", "--op-iters", "1", "--dump-outputs", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        d = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
        assert d["steps"] == 3 and d["timed_blocks"] == 1
        assert sorted(os.listdir(out)) == ["y.npy"]
        y = np.load(out / "y.npy")
        assert y.dtype == np.float32 and y.shape == (2, 3, 32, 32) and np.isfinite(y).all()
        ys.append(y)
    assert np.array_equal(ys[0], ys[1])
    from conftest import load_keys
    from emu import build_emu
    from vtoonify_amd import _lib, synth
    from vtoonify_amd.engine import VToonifyEngine
    _lib.use_library(build_emu.build())
    eng = VToonifyEngine(synth.synth_state_dict(load_keys("T"), 0), "toonify", 256, torch.bfloat16, torch.device("cpu"))
    want = [eng.forward(synth.synth_frames(2, 8, 8, seed=i), synth.synth_style(seed=17), 0.5).float().numpy()
            for i in (1, 2)]
    assert np.array_equal(ys[0], want[1]) and not np.array_equal(ys[0], want[0])


def test_bench_two_ranks_dry_run_gloo_emulation():
    """The N > 1 control flow of bench.py (one process per rank under torch.distributed.run, weight / style
    broadcast, equal block counts on every rank, MAX-over-ranks timing, extra keys, rank-0-only sections, final
    barrier) with gloo on CPU and the host-emulation kernels: `--dry-run-emu` is a TEST MODE, its numbers mean
    nothing (the line says "data": "dry-run").  A hang or a mismatched collective here is what would lose the
    driver's 8-GPU scaling leg."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29541", os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1",
           "--warmup", "1", "--dry-run-emu", "--height", "8", "--width", "8", "--lanes", "1", "--min-seconds", "0",
           "--dtype", "bf16", "--backbone", "toonify", "--batch", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, from rank 0"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["data"] == "dry-run" and d["scaling"] == "weak"
    assert d["config"]["parallelism"] == "frame-parallel x2" and d["value"] > 0
    for k in ("batch1", "config3", "single_stream", "module_call"):
        assert d[k]["value"] > 0, k
    assert d["cpu_baseline"] is None
