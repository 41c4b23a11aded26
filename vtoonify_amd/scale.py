"""--scale_image on the GPU: the reference's per-frame low-pass filter, resize and crop (style_transfer.py:113-127,150-155;
util.py:163-188) as ONE kernel launch per batch over source-size uint8 frames (csrc/frame_scale.hip, vt_frame_scale_crop).

    params = crop_parameters(landmarks, frame.shape[:2], padding)      # the first frame's eye distance fixes them
    sc = ScaleCrop(params, Hs, Ws).to(device)
    crop = sc(frame)                                                   # one host frame: upload slab, launch, download
    VideoToonifier(engine, style, d_s, prescale=sc).run(source_size_frames, sink)

The arithmetic is integer arithmetic on uint8 pixels: `ScaleCrop.host` is its vectorised numpy form (the
`--cpu` path), the kernel matches it bit for bit.  The host builds the resize tables once; only the source rows the crop and
its blur halo read -- the row slab [row0, row0 + rows) -- are staged and uploaded per frame.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

TAPS = (32, 96, 96, 32)          # [1,3,3,1]/8 in 8 fractional bits, at offsets -2, -1, 0, +1 (cv2.sepFilter2D, even kernel)
OFFSETS = (-2, -1, 0, 1)


class CropParams(NamedTuple):
    scale: float
    h: int          # the resized frame
    w: int
    left: int       # the crop inside it
    right: int
    top: int
    bottom: int
    passes: int     # blur passes in front of the resize


def crop_parameters(lm: np.ndarray, shape: Sequence[int], padding: Sequence[int]) -> CropParams:
    """util.py:163-188 (get_video_crop_parameter) as a pure function: 64 pixels between the eyes, `padding` (left, right, top,
    bottom) around their centre, edges on multiples of 8; style_transfer.py:150-155 for the number of blur passes."""
    lm = np.asarray(lm, dtype=np.float64)
    if lm.shape != (68, 2):
        raise ValueError(f"landmarks must be (68,2), got {lm.shape}")
    Hs, Ws = int(shape[0]), int(shape[1])
    pl, pr, pt, pb = padding
    eye_l, eye_r = lm[36:42], lm[42:48]
    scale = 64.0 / (np.mean(eye_r[:, 0]) - np.mean(eye_l[:, 0]))
    cx, cy = ((np.mean(eye_r, axis=0) + np.mean(eye_l, axis=0)) / 2) * scale
    h, w = round(Hs * scale), round(Ws * scale)
    left = max(round(cx - pl), 0) // 8 * 8
    right = min(round(cx + pr), w) // 8 * 8
    top = max(round(cy - pt), 0) // 8 * 8
    bottom = min(round(cy + pb), h) // 8 * 8
    passes = 0 if scale > 0.75 else 1 if scale > 0.375 else 2
    return CropParams(float(scale), int(h), int(w), int(left), int(right), int(top), int(bottom), passes)


def _axis_table(lo: int, hi: int, dst: int, src: int, horizontal: bool) -> np.ndarray:
    """(hi-lo,4) int32: i0, i1, w0, w1 of output positions [lo, hi) of an axis resized src -> dst (cv2.resize INTER_LINEAR on
    8-bit images: coordinates in float32, weights of 2048 rounded half to even)."""
    sc = 1.0 / (dst / src)
    f = ((np.arange(lo, hi, dtype=np.float64) + 0.5) * sc - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = (f - i.astype(np.float32)).astype(np.float32)
    if horizontal:
        low, high = i < 0, i >= src - 1
        f[low | high] = 0
        i[low] = 0
        i[high] = src - 1
        i0, i1 = i, np.minimum(i + 1, src - 1)
    else:
        i0, i1 = np.clip(i, 0, src - 1), np.clip(i + 1, 0, src - 1)
    w0 = np.rint((np.float32(1) - f).astype(np.float32) * np.float32(2048))
    w1 = np.rint(f * np.float32(2048))
    return np.stack([i0, i1, w0, w1], 1).astype(np.int32)


def resize_tables(p: CropParams, Hs: int, Ws: int) -> Tuple[np.ndarray, np.ndarray]:
    """xtab (W,4) = x0, x1, a0, a1 per output column; ytab (H,4) = y0, y1, b0, b1 per output row."""
    return _axis_table(p.left, p.right, p.w, Ws, True), _axis_table(p.top, p.bottom, p.h, Hs, False)


def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _expand(lo: int, hi: int, n: int) -> Tuple[int, int]:
    """What one blur pass over [lo, hi] reads of an axis of n samples: [lo-2, hi+1] reflected into the frame (fs_expand)."""
    a, b = lo - 2, hi + 1
    lo2, hi2 = max(a, 0), min(b, n - 1)
    if a < 0:
        hi2 = max(hi2, -a)
    if b > n - 1:
        lo2 = min(lo2, 2 * (n - 1) - b)
    return lo2, hi2


def blur_pass(P: np.ndarray) -> np.ndarray:
    """One [1,3,3,1]/8 x [1,3,3,1]/8 pass over an (Hs,Ws,3) uint8 frame, reflect-101 borders, one rounding."""
    Hs, Ws = P.shape[:2]
    k, off = np.array(TAPS, dtype=np.int32), np.array(OFFSETS)
    rx = _reflect(np.arange(Ws)[:, None] + off[None], Ws)
    ry = _reflect(np.arange(Hs)[:, None] + off[None], Hs)
    Pi = P.astype(np.int32)
    rows = sum(k[j] * Pi[:, rx[:, j]] for j in range(4))
    both = sum(k[i] * rows[ry[:, i]] for i in range(4))
    return ((both + 32768) >> 16).astype(np.uint8)


def _stream(t: torch.Tensor):
    if t.device.type == "cuda":
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return C.c_void_p(0)


class ScaleCrop:
    """The crop of one video: tables (on the device once uploaded), row slab, kernel launch and host form."""

    def __init__(self, params: CropParams, Hs: int, Ws: int, device=None):
        self.params, self.Hs, self.Ws = params, int(Hs), int(Ws)
        self.H, self.W, self.passes = params.bottom - params.top, params.right - params.left, params.passes
        if self.H <= 0 or self.W <= 0:
            raise _lib.VtError(f"--scale_image: empty crop {self.H} x {self.W} (rows {params.top}:{params.bottom}, columns "
                               f"{params.left}:{params.right} of the {params.h} x {params.w} resized frame)")
        if self.passes and (self.Hs < 3 or self.Ws < 3):
            raise _lib.VtError("--scale_image: a blur pass needs a frame of at least 3 x 3")
        self.xtab, self.ytab = resize_tables(params, self.Hs, self.Ws)
        lo, hi = int(self.ytab[:, :2].min()), int(self.ytab[:, :2].max())
        for _ in range(self.passes):
            lo, hi = _expand(lo, hi, self.Hs)
        self.row0, self.rows = lo, hi - lo + 1
        self.device = None
        self._tables = None
        if device is not None:
            self.to(device)

    def to(self, device) -> "ScaleCrop":
        self._tables = (torch.from_numpy(self.xtab).to(device), torch.from_numpy(self.ytab).to(device))
        self.device = self._tables[0].device
        return self

    def slab(self, frame: np.ndarray) -> np.ndarray:
        """The contiguous rows of a source frame that the crop reads."""
        if frame.shape != (self.Hs, self.Ws, 3) or frame.dtype != np.uint8:
            raise _lib.VtError(f"--scale_image: frame {frame.shape} {frame.dtype}, expected ({self.Hs},{self.Ws},3) uint8")
        return frame[self.row0:self.row0 + self.rows]

    def apply(self, src: torch.Tensor, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """src (n,rows,Ws,3) uint8 row slabs, or (n,Hs,Ws,3) whole frames, on the device -> out (n,H,W,3) uint8
        (vt_frame_scale_crop, one launch)."""
        if self._tables is None or src.device != self.device:
            raise _lib.VtError("ScaleCrop.apply: call .to(device) first; frames must be on that device")
        if src.dtype != torch.uint8 or src.ndim != 4 or src.shape[2] != self.Ws or src.shape[3] != 3 or \
                src.shape[1] not in (self.rows, self.Hs):
            raise _lib.VtError(f"ScaleCrop.apply: frames must be (n,{self.rows} or {self.Hs},{self.Ws},3) uint8")
        src = src.contiguous()
        n, rows = src.shape[0], src.shape[1]
        row0 = self.row0 if rows == self.rows else 0
        if out is None:
            out = torch.empty((n, self.H, self.W, 3), dtype=torch.uint8, device=src.device)
        elif tuple(out.shape) != (n, self.H, self.W, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
            raise _lib.VtError(f"ScaleCrop.apply: out must be contiguous ({n},{self.H},{self.W},3) uint8")
        xt, yt = self._tables
        _lib.check(_lib.lib().vt_frame_scale_crop(C.c_void_p(out.data_ptr()), C.c_void_p(src.data_ptr()), n, rows, row0,
                                                  self.Hs, self.Ws, self.passes, C.c_void_p(xt.data_ptr()),
                                                  C.c_void_p(yt.data_ptr()), self.H, self.W,
                                                  _stream(src) if stream is None else stream), "vt_frame_scale_crop")
        return out

    def __call__(self, frame: np.ndarray) -> np.ndarray:
        """One host frame through the kernel: upload its slab, launch, download."""
        if self.device is None:
            raise _lib.VtError("ScaleCrop: call .to(device) first")
        d = torch.from_numpy(np.array(self.slab(frame))[None]).to(self.device)       # (a copy: memory-mapped clips are read-only)
        return self.apply(d)[0].cpu().numpy()

    def host(self, frame: np.ndarray) -> np.ndarray:
        """The same crop in numpy (`--cpu`): the arithmetic of DESIGN.md 4.8, vectorised."""
        self.slab(frame)
        Q = frame
        for _ in range(self.passes):
            Q = blur_pass(Q)
        x0, x1, a0, a1 = (self.xtab[:, j] for j in range(4))
        y0, y1, b0, b1 = (self.ytab[:, j][:, None, None] for j in range(4))
        a0, a1 = a0[None, :, None], a1[None, :, None]
        Qi = Q.astype(np.int32)
        r0, r1 = Qi[self.ytab[:, 0]], Qi[self.ytab[:, 1]]
        h0 = a0 * r0[:, x0] + a1 * r0[:, x1]
        h1 = a0 * r1[:, x0] + a1 * r1[:, x1]
        return ((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)
