#!/usr/bin/env python3
"""Frames/s of the flicker-reduction pre-pass on one box: the whole-clip loop (smooth_parsing_maps + raft_flow_fn + one
BiSeNet pass per frame over a clip resident as fp32) against the streaming smooth.ParsingSmoother, alternating.

    python tools/smooth_bench.py [--size 256] [--window 5] [--frames 16] [--reps 5] > profiles/smooth_bench.txt

--size is the frame size BEFORE the doubling (256 -> 512 x 512 as in smooth_parsing_map.py:128).  One warm-up run of each
arm, then `reps` alternating timed runs (whole, stream, whole, stream ...), each bracketed by a device synchronise;
reported: median and min..max frames/s per arm, for fp32 and for bf16 RAFT.  Synthetic weights (timing does not depend
on the values; 20 iterations always run).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vtoonify_amd import smooth, synth  # noqa: E402
from vtoonify_amd.bisenet import BiSeNetEngine  # noqa: E402
from vtoonify_amd.raft import RaftEngine  # noqa: E402


def _shapes(tag):
    with open(os.path.join(REPO, "tests", "golden", f"keys_{tag}.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    base = g.integers(0, 256, (a.size + a.frames, a.size + a.frames, 3), dtype=np.uint8)
    frames = torch.from_numpy(np.stack([base[t:t + a.size, t:t + a.size] for t in range(a.frames)], 0).copy())
    bise = BiSeNetEngine(synth.synth_state_dict(_shapes("bisenet"), 0), 19, torch.float32, dev)
    for dtype in (torch.float32, torch.bfloat16):
        raft = RaftEngine(synth.synth_state_dict(_shapes("raft"), 0), dtype, dev)

        class Module:
            def __call__(self, i1, i2, iters=12, test_mode=True):
                lo, ups = raft.forward(i1, i2, iters=iters)
                return lo, ups[-1]

        def whole():
            x = (frames.to(dev).permute(0, 3, 1, 2).float().div(255) - 0.5) / 0.5
            Is = torch.nn.functional.interpolate(x.flip(1), scale_factor=2, mode="bilinear", align_corners=False)
            Ps = torch.cat([bise.forward(2 * Is[i:i + 1])[0] for i in range(a.frames)], 0)
            return smooth.smooth_parsing_maps(Is, Ps, smooth.raft_flow_fn(Module(), a.iters), a.window)

        def stream():
            sm = smooth.ParsingSmoother(raft, bise, a.window, iters=a.iters, bgr=True)
            return torch.cat(list(sm.smooth([frames])), 0)

        def timed(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return a.frames / (time.perf_counter() - t)

        whole(), stream()
        fps = {"whole": [], "stream": []}
        for _ in range(a.reps):
            fps["whole"].append(timed(whole))
            fps["stream"].append(timed(stream))
        for arm, v in fps.items():
            print(f"RAFT {str(dtype).split('.')[1]:8s} {arm:6s} {2 * a.size}x{2 * a.size} window {a.window} {a.frames} frames x "
                  f"{a.reps} runs: median {statistics.median(v):.2f} frames/s (min {min(v):.2f}, max {max(v):.2f})", flush=True)


if __name__ == "__main__":
    main()
