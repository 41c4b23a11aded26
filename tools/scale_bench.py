#!/usr/bin/env python3
"""--scale_image on the GPU, measured: the blur + resize + crop kernel (vt_frame_scale_crop) and the video driver with it.

    python tools/scale_bench.py [--launches 50] [--driver_frames 96] [--no_driver] > profiles/scale_image.json

Kernel: 1080p and 4K sources at scales 0.3, 0.6 and 0.9 (2, 1 and 0 blur passes), batch of 4, the crop the reference's default
--padding 200 gives around the frame centre.  Event timing over `launches` back-to-back launches after a warm-up (queued behind a blocker: event_time below); GB/s of ALGORITHMIC bytes
(n*rows*Ws*3 read + n*H*W*3 written) next to vt_frame_unpack's figure (n*H*W*15) from the same process -- the ratio to that
streaming kernel is the number to read.
Driver: VideoToonifier(prescale=...) on 1080p source frames against VideoToonifier() on pre-cropped frames of the same crop
size (the path without --scale_image), alternating, three runs each, frames/s host to host.  Synthetic weights, bf16.
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
from vtoonify_amd import _lib, synth, video  # noqa: E402
from vtoonify_amd.scale import CropParams, ScaleCrop  # noqa: E402


def centre_crop(Hs, Ws, scale, pad=200):
    """The crop of a face at the frame centre with --padding 200 200 200 200 (util.py:163-188)."""
    h, w = round(Hs * scale), round(Ws * scale)
    cx, cy = w / 2, h / 2
    left, right = max(round(cx - pad), 0) // 8 * 8, min(round(cx + pad), w) // 8 * 8
    top, bottom = max(round(cy - pad), 0) // 8 * 8, min(round(cy + pad), h) // 8 * 8
    return CropParams(scale, h, w, left, right, top, bottom, 0 if scale > 0.75 else 1 if scale > 0.375 else 2)


def event_time(fn, launches, warmup=5):
    """Seconds per launch on the device: the launches are queued on a side stream BEHIND a few milliseconds of other work, so
    the two events bracket `launches` kernels running back to back -- vt_frame_scale_crop's launcher copies its tables to the
    host first and would otherwise be timed at the host's pace, not the kernel's.  Returns (seconds, queued): `queued` says
    that the host had issued every launch before the device reached the first (the figure is device time only then)."""
    st = torch.cuda.Stream()
    big = event_time.big
    with torch.cuda.stream(st):
        for _ in range(warmup):
            fn()
        st.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(24):
            big.add_(1.0)
        a.record(st)
        for _ in range(launches):
            fn()
        b.record(st)
        queued = not a.query()
        st.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches, queued


def kernel_rows(dev, launches, n=4):
    g = np.random.default_rng(0)
    y = torch.from_numpy(g.standard_normal((n, 3, 1024, 1024)).astype(np.float32)).to(dev)
    o = torch.empty((n, 1024, 1024, 3), dtype=torch.uint8, device=dev)
    event_time.big = torch.zeros(1 << 28, dtype=torch.float32, device=dev)      # 1 GiB: ~0.4 ms per pass
    t, q = event_time(lambda: video.frame_unpack(y, True, out=o), launches)
    unpack = {"kernel": "vt_frame_unpack", "n": n, "hw": [1024, 1024], "seconds": t, "queued_behind_blocker": q,
              "gbps": n * 1024 * 1024 * 15 / t / 1e9}
    rows = []
    for name, (Hs, Ws) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
        for scale in (0.3, 0.6, 0.9):
            sc = ScaleCrop(centre_crop(Hs, Ws, scale), Hs, Ws).to(dev)
            src = torch.from_numpy(g.integers(0, 256, (n, sc.rows, Ws, 3), dtype=np.uint8)).to(dev)
            out = torch.empty((n, sc.H, sc.W, 3), dtype=torch.uint8, device=dev)
            t, q = event_time(lambda: sc.apply(src, out=out), launches)
            with torch.cuda.stream(torch.cuda.Stream()):           # host time of a call (table check included), device not waited for
                t0 = time.perf_counter()
                for _ in range(launches):
                    sc.apply(src, out=out)
                host = (time.perf_counter() - t0) / launches
            torch.cuda.synchronize()
            nbytes = n * sc.rows * Ws * 3 + n * sc.H * sc.W * 3
            rows.append({"source": name, "scale": scale, "passes": sc.passes, "n": n, "crop": [sc.H, sc.W], "slab_rows": sc.rows,
                         "algorithmic_bytes": nbytes, "seconds": t, "queued_behind_blocker": q, "host_seconds_per_call": host, "gbps": nbytes / t / 1e9,
                         "ratio_to_frame_unpack": nbytes / t / 1e9 / unpack["gbps"]})
    return unpack, rows


def driver_rows(dev, frames_n, runs=3, batch=4, depth=3):
    with open(os.path.join(REPO, "tests", "golden", "keys_D.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    from vtoonify_amd.engine import VToonifyEngine
    sd = {k: v.to(dev) for k, v in synth.synth_state_dict(shapes, 0).items()}
    eng = VToonifyEngine(sd, "dualstylegan", 256, torch.bfloat16, dev)
    style = synth.synth_style(seed=5).to(dev)
    Hs, Ws = 1080, 1920
    sc = ScaleCrop(centre_crop(Hs, Ws, 0.6), Hs, Ws).to(dev)
    g = np.random.default_rng(1)
    srcs = [g.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(8)]
    crops = [sc(f) for f in srcs]
    maps = (g.standard_normal((19, sc.H, sc.W)) * 4).astype(np.float32)
    arms = {"prescale_1080p": (video.VideoToonifier(eng, style, 0.5, batch_size=batch, depth=depth, prescale=sc), srcs),
            "precropped": (video.VideoToonifier(eng, style, 0.5, batch_size=batch, depth=depth), crops)}
    rates = {k: [] for k in arms}
    for r in range(runs + 1):                  # run 0 warms both arms up (plans, graphs, pinned buffers)
        for k, (vt, fr) in arms.items():
            n = 2 * batch * depth if r == 0 else frames_n
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vt.run(((fr[i % len(fr)], maps) for i in range(n)), lambda i, o: None)
            torch.cuda.synchronize()
            if r:
                rates[k].append(n / (time.perf_counter() - t0))
    return {"source": [Hs, Ws], "scale": 0.6, "crop": [sc.H, sc.W], "slab_rows": sc.rows, "frames": frames_n, "batch": batch,
            "depth": depth, "frames_per_s": rates, "median": {k: statistics.median(v) for k, v in rates.items()},
            "scale_on_host": "not measured (needs cv2)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--driver_frames", type=int, default=96)
    ap.add_argument("--no_driver", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.use_library(_lib.DEFAULT_LIB)
    unpack, rows = kernel_rows(dev, max(a.launches, 50))
    rep = {"frame_unpack": unpack, "frame_scale_crop": rows}
    if not a.no_driver:
        rep["driver"] = driver_rows(dev, a.driver_frames)
    print(json.dumps(rep, indent=1))


if __name__ == "__main__":
    main()
