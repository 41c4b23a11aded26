#!/usr/bin/env python3
"""`smooth_parsing_map.py` on MI355X: the reference's command line over the streaming pre-pass (smooth.ParsingSmoother).

    python tools/smooth_parsing_map_amd.py --video_path clip.mp4 --window_size 5 --output_path ./output/
    python tools/style_transfer_amd.py --content clip.mp4 --video --parsing_map_path ./output/clip_parsingmap.npy ...

The five options of the reference (smooth_parsing_map.py:21-27) keep their names, types and defaults; the output is the
reference's `<basename>_parsingmap.npy`, (N,19,H,W) float32 (:169-170).  Frames are read a chunk at a time and device
memory is bounded by the window (see ParsingSmoother), so the clip's length does not matter; the output file is a
memory-mapped .npy written frame by frame.

Sources as for style_transfer_amd.py (tools/frame_sources.py): a video file through cv2 when importable, an (N,H,W,3) uint8
.npy, or a directory of .npy frames.  `--raft_path synthetic` / `--faceparsing_path synthetic` build seeded random
weights of the reference's schemas.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frame_sources import open_source  # noqa: E402
from vtoonify_amd import smooth, synth  # noqa: E402
from vtoonify_amd.bisenet import BiSeNet  # noqa: E402
from vtoonify_amd.raft import RAFT  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Smooth Parsing Maps")
    # ---- the reference's options, verbatim (smooth_parsing_map.py:21-27) ----
    p.add_argument("--window_size", type=int, default=5, help="temporal window size")
    p.add_argument("--faceparsing_path", type=str, default="./checkpoint/faceparsing.pth", help="path of the face parsing model")
    p.add_argument("--raft_path", type=str, default="./checkpoint/raft-things.pth", help="path of the RAFT model")
    p.add_argument("--video_path", type=str, help="path of the target video")
    p.add_argument("--output_path", type=str, default="./output/", help="path of the output parsing maps")
    # ---- additions of this driver ----
    p.add_argument("--precision", choices=["fp32", "bf16", "fp16"], default="fp32",
                   help="arithmetic of RAFT and BiSeNet (fp32 = the reference's; the fusion is always fp32)")
    p.add_argument("--frame_order", choices=["bgr", "rgb"], default="bgr", help="channel order of .npy frames (cv2 files are BGR)")
    p.add_argument("--max_frames", type=int, default=None, help="stop after this many frames")
    p.add_argument("--chunk", type=int, default=8, help="frames read and uploaded at a time")
    p.add_argument("--seed", type=int, default=0, help="seed of `synthetic` weights")
    p.add_argument("--iters", type=int, default=20, help="RAFT iterations (20 = smooth_parsing_map.py:154)")
    return p


def _shapes(tag):
    with open(os.path.join(REPO, "tests", "golden", f"keys_{tag}.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


def load_models(opt, device, dtype):
    raft = RAFT(argparse.Namespace(model=opt.raft_path, small=False, mixed_precision=False, alternate_corr=False),
                compute_dtype=dtype)
    if opt.raft_path.startswith("synthetic"):
        raft.load_state_dict(synth.synth_state_dict(_shapes("raft"), opt.seed))
    else:       # saved from nn.DataParallel (smooth_parsing_map.py:97-100)
        sd = torch.load(opt.raft_path, map_location="cpu")
        raft.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()})
    par = BiSeNet(n_classes=19, compute_dtype=dtype)
    if opt.faceparsing_path.startswith("synthetic"):
        par.load_state_dict(synth.synth_state_dict(_shapes("bisenet"), opt.seed))
    else:
        par.load_state_dict(torch.load(opt.faceparsing_path, map_location="cpu"))
    return raft.to(device).eval(), par.to(device).eval()


def main(argv=None, device=None) -> dict:
    """Returns a small report (frames, seconds, output path).  `device` is for tests (host emulation)."""
    opt = build_parser().parse_args(argv)
    print("Load options")
    for k, v in sorted(vars(opt).items()):
        print(f"{k}: {v}")
    print("*" * 98, flush=True)
    if not opt.video_path:
        raise SystemExit("--video_path is required")
    device = torch.device("cuda", 0) if device is None else torch.device(device)
    src = open_source(opt.video_path, True, opt.frame_order)
    n = len(src) if opt.max_frames is None else min(len(src), opt.max_frames)
    raft, par = load_models(opt, device, {"bf16": torch.bfloat16, "fp16": torch.float16}.get(opt.precision, torch.float32))
    print("Load models successfully!", flush=True)
    sm = smooth.ParsingSmoother(raft, par, opt.window_size, iters=opt.iters, bgr=src.bgr)
    os.makedirs(opt.output_path, exist_ok=True)
    basename = os.path.basename(opt.video_path.rstrip("/")).split(".")[0]
    out_path = os.path.join(opt.output_path, basename + "_parsingmap.npy")
    out, done, t0 = None, 0, time.time()

    def chunks():
        buf = []
        for fr in src.frames(0, n):
            buf.append(fr)
            if len(buf) == opt.chunk:
                yield torch.from_numpy(np.stack(buf, 0))
                buf = []
        if buf:
            yield torch.from_numpy(np.stack(buf, 0))

    for p in sm.smooth(chunks()):
        if out is None:
            out = np.lib.format.open_memmap(out_path, mode="w+", dtype=np.float32, shape=(n,) + tuple(p.shape[1:]))
        out[done] = p[0].cpu().numpy()
        done += 1
    if out is None:
        raise SystemExit(f"{opt.video_path}: no frames")
    out.flush()
    del out
    if done < n:      # a container that announces more frames than it delivers: keep what exists, say so
        kept = np.load(out_path, mmap_mode="r")[:done]
        np.save(out_path + ".tmp.npy", kept)
        del kept
        os.replace(out_path + ".tmp.npy", out_path)
        print(f"[warning] {opt.video_path}: {n} frames announced, {done} read; {out_path} holds {done}", flush=True)
    dt = time.time() - t0
    print(f"Done!  {done} frames in {dt:.2f} s ({done / max(dt, 1e-9):.2f} frames/s incl. I/O), peak {sm.peak_slots} "
          f"frames resident -> {out_path}", flush=True)
    return {"frames": done, "seconds": dt, "output": out_path, "peak_slots": sm.peak_slots}


if __name__ == "__main__":
    main()
