#!/usr/bin/env python3
"""Time of the face alignment for the style encoder (vtoonify_amd/align.py FaceAligner) per case, on one GPU.

    python tools/align_bench.py [--iters 20] [--warmup 3] [--out profiles/align_bench.json]

Each case of tests/align_cases.py, plus a 375x500 and an 1125x1500 portrait (face inside / at the border / close-up), goes
through FaceAligner from a HOST frame: plan, tables, upload of the rows that are read, kernels.  Timed with events after a
warm-up, synchronised before reading; the wall time per call (host work included) is reported beside it.  Where Pillow and
scipy are importable the same inputs also go through a plain Pillow / scipy restatement of the reference's host path on this
machine's CPU.  One JSON line goes to --out.  The figure gates nothing: it is set against the host path, never against
earlier runs of the kernels.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import align_cases as AC  # noqa: E402
from vtoonify_amd import align as A  # noqa: E402


def inputs():
    out = {name: AC.case(name) for name in AC.CASES}
    out["375x500 inside"] = (AC.image(375, 500, 21), AC.landmarks((250, 160), 55, 0.05))
    out["375x500 border"] = (AC.image(375, 500, 22), AC.landmarks((60, 120), 60, -0.1))
    out["1125x1500 close-up"] = (AC.image(1125, 1500, 23), AC.landmarks((750, 480), 330, 0.03))
    return out


def host_reference(frame, lm):
    """The reference's host path with Pillow and scipy, from the plan of vtoonify_amd/align.py (same branches, same numbers)."""
    import scipy.ndimage
    from PIL import Image
    p = A.align_parameters(lm, frame.shape)
    img = Image.fromarray(frame)
    if p.shrink > 1:
        img = img.resize(p.rsize, Image.LANCZOS)
    if p.crop is not None:
        img = img.crop(p.crop)
    if p.pad is not None:
        pad = p.pad
        a = np.pad(np.float32(img), ((pad[1], pad[3]), (pad[0], pad[2]), (0, 0)), "reflect")
        h, w, _ = a.shape
        y, x, _ = np.ogrid[:h, :w, :1]
        mask = np.maximum(1.0 - np.minimum(np.float32(x) / pad[0], np.float32(w - 1 - x) / pad[2]),
                          1.0 - np.minimum(np.float32(y) / pad[1], np.float32(h - 1 - y) / pad[3]))
        a += (scipy.ndimage.gaussian_filter(a, [p.sigma, p.sigma, 0]) - a) * np.clip(mask * 3.0 + 1.0, 0.0, 1.0)
        a += (np.median(a, axis=(0, 1)) - a) * np.clip(mask, 0.0, 1.0)
        img = Image.fromarray(np.uint8(np.clip(np.rint(a), 0, 255)))
    quad = getattr(Image, "Transform", Image).QUAD
    bil = getattr(Image, "Resampling", Image).BILINEAR
    return np.asarray(img.transform((256, 256), quad, (p.quad + 0.5).flatten(), bil))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "align_bench.json"))
    opt = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    fa = A.FaceAligner(dev)
    try:
        import PIL  # noqa: F401
        import scipy  # noqa: F401
        have_host = True
    except ImportError:
        have_host = False
    rows = {}
    for name, (frame, lm) in inputs().items():
        plan = A.align_parameters(lm, frame.shape)
        for _ in range(opt.warmup):
            u8, _x = fa(frame, lm)
        torch.cuda.synchronize(dev)
        ev, wall = [], []
        for _ in range(opt.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            u8, _x = fa(frame, lm)
            b.record()
            torch.cuda.synchronize(dev)
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(a.elapsed_time(b))
        row = {"shape": list(frame.shape[:2]), "shrink": plan.shrink, "pad": plan.pad is not None, "size": list(plan.size),
               "gpu_event_ms_median": float(np.median(ev)), "gpu_event_ms_min": float(np.min(ev)),
               "wall_ms_median": float(np.median(wall))}
        if have_host:
            ref = host_reference(frame, lm)
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                host_reference(frame, lm)
                t.append((time.perf_counter() - t0) * 1e3)
            d = np.abs(ref.astype(np.int32) - u8.cpu().numpy().astype(np.int32))
            row.update(host_reference_ms_median=float(np.median(t)), max_abs_diff=int(d.max()), share_differing=float((d > 0).mean()))
        rows[name] = row
        print(name, json.dumps(row), flush=True)
    rec = {"tool": "align_bench", "device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(),
           "iters": opt.iters, "warmup": opt.warmup, "cases": rows}
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
