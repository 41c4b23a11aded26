"""Face alignment for the pSp style encoder from GIVEN landmarks (model/encoder/align_all_parallel.py:59-150, everything after
`get_landmark`): a plan computed on the host in float64 plus three kernels (csrc/face_align.hip, include/vtoonify_amd_align.h).

    plan = align_parameters(lm, frame.shape)                 # quad, shrink, crop, pad: the reference's lines 69-132
    crop_u8, x = FaceAligner(device)(frame_rgb_uint8, lm)    # (256,256,3) uint8 and (1,3,256,256) float32, on the device
    crop_u8 = align_face_host(frame_rgb_uint8, lm)           # the same arithmetic in numpy (`--cpu`)

The arithmetic is DESIGN.md 4.9: the Lanczos shrink and the quad transform are bit-exact against Pillow (integer and float64
arithmetic), the pad branch accumulates its Gaussian blur in float64 like scipy.ndimage and selects the exact median.  Neither
PIL nor scipy is imported here.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

OUTPUT_SIZE = 256                # output_size == transform_size of the reference: no final resize
PRECISION_BITS = 32 - 8 - 2      # Pillow's fixed-point coefficients of 8-bit resampling
MAX_RADIUS = 128                 # of the pad branch's blur on the device (VT_ALIGN_MAX_RADIUS)


class AlignPlan(NamedTuple):
    shrink: int
    rsize: Optional[Tuple[int, int]]            # (W, H) of the shrunk image; None when shrink <= 1
    crop: Optional[Tuple[int, int, int, int]]   # (x0, y0, x1, y1) in the (shrunk) image; None when the whole image is kept
    pad: Optional[Tuple[int, int, int, int]]    # (left, top, right, bottom); None when the pad branch is not taken
    sigma: float                                # of the pad branch's blur (qsize * 0.02)
    quad: np.ndarray                            # (4,2) float64 nw, sw, se, ne in the image the transform reads
    size: Tuple[int, int]                       # (h, w) of that image


def align_parameters(lm, shape: Sequence[int]) -> AlignPlan:
    """align_all_parallel.py:69-132 as a pure function of the 68 landmarks and the image shape (H, W[, 3]), in float64."""
    lm = np.asarray(lm, dtype=np.float64)
    if lm.shape != (68, 2):
        raise ValueError(f"landmarks must be (68,2), got {lm.shape}")
    H, W = int(shape[0]), int(shape[1])
    eye_left, eye_right = np.mean(lm[36:42], axis=0), np.mean(lm[42:48], axis=0)
    eye_avg = (eye_left + eye_right) * 0.5
    eye_to_eye = eye_right - eye_left
    mouth_avg = (lm[48] + lm[54]) * 0.5
    eye_to_mouth = mouth_avg - eye_avg

    x = eye_to_eye - np.flipud(eye_to_mouth) * [-1, 1]
    x /= np.hypot(*x)
    x *= max(np.hypot(*eye_to_eye) * 2.0, np.hypot(*eye_to_mouth) * 1.8)
    y = np.flipud(x) * [-1, 1]
    c = eye_avg + eye_to_mouth * 0.1
    quad = np.stack([c - x - y, c - x + y, c + x + y, c + x - y])
    qsize = np.hypot(*x) * 2
    if not np.isfinite(quad).all() or not qsize > 0:
        raise ValueError("landmarks give no oriented crop rectangle (eyes and mouth coincide)")

    w, h = W, H
    shrink = int(np.floor(qsize / OUTPUT_SIZE * 0.5))
    rsize = None
    if shrink > 1:
        rsize = (int(np.rint(float(W) / shrink)), int(np.rint(float(H) / shrink)))
        quad /= shrink
        qsize /= shrink
        w, h = rsize

    border = max(int(np.rint(qsize * 0.1)), 3)
    crop = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))),
            int(np.ceil(max(quad[:, 1]))))
    crop = (max(crop[0] - border, 0), max(crop[1] - border, 0), min(crop[2] + border, w), min(crop[3] + border, h))
    if crop[2] - crop[0] < w or crop[3] - crop[1] < h:
        if crop[2] <= crop[0] or crop[3] <= crop[1]:
            raise ValueError(f"the face lies outside the image: empty crop {crop} of a {w} x {h} image")
        quad -= crop[0:2]
        w, h = crop[2] - crop[0], crop[3] - crop[1]
    else:
        crop = None

    pad = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))),
           int(np.ceil(max(quad[:, 1]))))
    pad = (max(-pad[0] + border, 0), max(-pad[1] + border, 0), max(pad[2] - w + border, 0), max(pad[3] - h + border, 0))
    sigma = float(qsize * 0.02)
    if max(pad) > border - 4:
        pad = tuple(int(p) for p in np.maximum(pad, int(np.rint(qsize * 0.3))))
        if min(pad) < 1:
            raise ValueError(f"pad {pad}: the mask of the pad branch divides by a pad of 0")
        if max(pad[0], pad[2]) >= w or max(pad[1], pad[3]) >= h:
            raise ValueError(f"pad {pad} (left, top, right, bottom) reaches the side of the {w} x {h} image it reflects: "
                             "the face is too large for this image")
        quad += pad[:2]
        w, h = w + pad[0] + pad[2], h + pad[1] + pad[3]
    else:
        pad = None
    return AlignPlan(shrink, rsize, crop, pad, sigma, quad, (h, w))


# ------------------------------------------------------------------------------------------------------------- tables
def _lanczos3(x: float) -> float:
    if -3.0 <= x < 3.0:
        if x == 0.0:
            return 1.0
        a, b = x * math.pi, x / 3.0 * math.pi
        return (math.sin(a) / a) * (math.sin(b) / b)
    return 0.0


def lanczos_tables(n_in: int, n_out: int, lo: int = 0, hi: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's 8-bit LANCZOS coefficients of output positions [lo, hi) of an axis resized n_in -> n_out:
    bounds (n,2) int32 = first input index and tap count, coef (n,K) int32 = weights of 2**22 (zero beyond the count)."""
    hi = n_out if hi is None else hi
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ss = 1.0 / fs
    rows, bounds = [], []
    for xx in range(lo, hi):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        k = [_lanczos3((x - center + 0.5) * ss) for x in range(xmin, xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        rows.append([int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in k])
        bounds.append((xmin, xmax - xmin))
    K = max(len(r) for r in rows)
    coef = np.zeros((len(rows), K), dtype=np.int32)
    for i, r in enumerate(rows):
        coef[i, :len(r)] = r
    return np.array(bounds, dtype=np.int32).reshape(-1, 2), coef


def gaussian_taps(sigma: float) -> np.ndarray:
    """scipy.ndimage.gaussian_filter's kernel, one side: taps[j] is the weight at offsets +-j, j = 0..int(4 sigma + 0.5)."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:], dtype=np.float64)


def quad_coefficients(quad: np.ndarray, size: int) -> np.ndarray:
    """The eight coefficients Pillow's Image.transform(QUAD) derives from (quad + 0.5).flatten() for a size x size output."""
    nw, sw, se, ne = (quad + 0.5)
    As = At = 1.0 / size
    return np.array([nw[0], (ne[0] - nw[0]) * As, (sw[0] - nw[0]) * At, (se[0] - sw[0] - ne[0] + nw[0]) * As * At,
                     nw[1], (ne[1] - nw[1]) * As, (sw[1] - nw[1]) * At, (se[1] - sw[1] - ne[1] + nw[1]) * As * At],
                    dtype=np.float64)


class _Region(NamedTuple):
    x0: int
    y0: int
    x1: int
    y1: int


def _region(plan: AlignPlan, W: int, H: int) -> _Region:
    """The rectangle of the (shrunk) image that the later stages read."""
    if plan.crop is not None:
        return _Region(*plan.crop)
    w, h = plan.rsize if plan.rsize is not None else (W, H)
    return _Region(0, 0, w, h)


# ---------------------------------------------------------------------------------------------------------- host form
def resample_host(src: np.ndarray, row0: int, xb, xk, yb, yk) -> np.ndarray:
    """The two Lanczos passes in integer numpy: src holds source rows [row0, row0 + len(src)) -> (len(yb), len(xb), 3) uint8."""
    def clip8(acc):
        return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)

    r0, r1 = int(yb[:, 0].min()), int((yb[:, 0] + yb[:, 1]).max())
    P = src[r0 - row0:r1 - row0].astype(np.int64)
    acc = np.full((P.shape[0], len(xb), 3), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for k in range(xk.shape[1]):
        idx = np.minimum(xb[:, 0] + k, src.shape[1] - 1)           # (beyond the count the coefficient is zero)
        acc += xk[:, k].astype(np.int64)[None, :, None] * P[:, idx]
    T = clip8(acc).astype(np.int64)
    acc = np.full((len(yb), len(xb), 3), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for k in range(yk.shape[1]):
        idx = np.minimum(yb[:, 0] + k - r0, T.shape[0] - 1)
        acc += yk[:, k].astype(np.int64)[:, None, None] * T[idx]
    return clip8(acc)


def blur_axis_host(img: np.ndarray, taps: np.ndarray, axis: int) -> np.ndarray:
    """One axis of scipy.ndimage.gaussian_filter on a float32 image: boundary 'reflect' (the edge sample repeats), the line
    summed in float64 from the centre tap, then pairs from the outermost inwards, stored as float32."""
    r = len(taps) - 1
    padw = [(0, 0)] * img.ndim
    padw[axis] = (r, r)
    ext = np.pad(img.astype(np.float64), padw, mode="symmetric")
    n = img.shape[axis]

    def at(off):
        s = [slice(None)] * img.ndim
        s[axis] = slice(r + off, r + off + n)
        return ext[tuple(s)]

    acc = at(0) * taps[0]
    for j in range(r, 0, -1):
        acc = acc + (at(-j) + at(j)) * taps[j]
    return acc.astype(np.float32)


def _key(a: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def pad_blend_host(view: np.ndarray, pad: Sequence[int], taps: np.ndarray) -> np.ndarray:
    """The pad branch (align_all_parallel.py:133-141) on an (h0,w0,3) uint8 view, float32 throughout: (h,w,3) uint8."""
    pl, pt, pr, pb = (int(p) for p in pad)
    f1 = np.float32(1.0)
    img = np.pad(view.astype(np.float32), ((pt, pb), (pl, pr), (0, 0)), "reflect")
    h, w, _ = img.shape
    y, x = np.arange(h, dtype=np.float32)[:, None, None], np.arange(w, dtype=np.float32)[None, :, None]
    mx = np.minimum(x / np.float32(pl), (np.float32(w - 1) - x) / np.float32(pr))
    my = np.minimum(y / np.float32(pt), (np.float32(h - 1) - y) / np.float32(pb))
    mask = np.maximum(f1 - mx, f1 - my).astype(np.float32)
    blur = blur_axis_host(blur_axis_host(img, taps, 0), taps, 1)
    img = img + (blur - img) * np.clip(mask * np.float32(3.0) + f1, np.float32(0), f1)
    flat = img.reshape(-1, 3)
    n = flat.shape[0]
    med = np.empty(3, dtype=np.float32)
    for c in range(3):
        order = np.argsort(_key(flat[:, c]), kind="stable")
        a, b = flat[order[(n - 1) // 2], c], flat[order[n // 2], c]
        med[c] = (a + b) / np.float32(2.0)
    img = img + (med - img) * np.clip(mask, np.float32(0), f1)
    assert img.dtype == np.float32
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def quad_host(img: np.ndarray, a: np.ndarray, size: int) -> np.ndarray:
    """Image.transform((size, size), QUAD, ..., BILINEAR) on an (h,w,3) uint8 image from the eight coefficients: float64,
    truncated to uint8; pixels whose sample point lies outside the image are 0."""
    h, w = img.shape[:2]
    xo = (np.arange(size, dtype=np.float64) + 0.5)[None, :]
    yo = (np.arange(size, dtype=np.float64) + 0.5)[:, None]
    xin = a[0] + a[1] * xo + a[2] * yo + a[3] * xo * yo
    yin = a[4] + a[5] * xo + a[6] * yo + a[7] * xo * yo
    outside = (xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h)
    xin, yin = np.where(outside, 0.5, xin) - 0.5, np.where(outside, 0.5, yin) - 0.5
    x, y = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    x, y = x.astype(np.int64), y.astype(np.int64)
    x0, x1 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1)
    y0, y1 = np.clip(y, 0, h - 1), np.clip(y + 1, 0, h - 1)
    P = img.astype(np.float64)
    v1 = P[y0, x0] + (P[y0, x1] - P[y0, x0]) * dx
    v2 = P[y1, x0] + (P[y1, x1] - P[y1, x0]) * dx
    v = v1 + (v2 - v1) * dy
    out = v.astype(np.int64).astype(np.uint8)
    out[outside] = 0
    return out


def normalise_host(crop: np.ndarray) -> np.ndarray:
    """ToTensor + Normalize(0.5, 0.5) of the reference's transform: (1,3,S,S) float32."""
    x = crop.astype(np.float32).transpose(2, 0, 1)[None]
    return ((x / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)


def _shrink_tables(plan: AlignPlan, H: int, W: int):
    reg = _region(plan, W, H)
    xb, xk = lanczos_tables(W, plan.rsize[0], reg.x0, reg.x1)
    yb, yk = lanczos_tables(H, plan.rsize[1], reg.y0, reg.y1)
    return reg, xb, xk, yb, yk


def align_face_host(frame: np.ndarray, lm) -> np.ndarray:
    """align_face of the reference on an (H,W,3) uint8 RGB frame with the landmarks given: (256,256,3) uint8, numpy only."""
    frame = np.asarray(frame)
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise ValueError(f"frame must be (H,W,3) uint8, got {frame.shape} {frame.dtype}")
    H, W = frame.shape[:2]
    plan = align_parameters(lm, frame.shape)
    if plan.shrink > 1:
        reg, xb, xk, yb, yk = _shrink_tables(plan, H, W)
        img = resample_host(frame, 0, xb, xk, yb, yk)
    else:
        reg = _region(plan, W, H)
        img = frame[reg.y0:reg.y1, reg.x0:reg.x1]
    if plan.pad is not None:
        img = pad_blend_host(img, plan.pad, gaussian_taps(plan.sigma))
    assert img.shape[:2] == plan.size
    return quad_host(img, quad_coefficients(plan.quad, OUTPUT_SIZE), OUTPUT_SIZE)


# ------------------------------------------------------------------------------------------------------------- device
def _stream(t: torch.Tensor):
    if t.device.type == "cuda":
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return C.c_void_p(0)


def resample(src: torch.Tensor, row0: int, Hs: int, xb, xk, yb, yk) -> torch.Tensor:
    """vt_align_resample_u8: src (rows,Ws,3) uint8 on the device = source rows [row0, row0+rows) -> (len(yb),len(xb),3)."""
    dev = src.device
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in (xb, xk, yb, yk)]
    out = torch.empty((len(yb), len(xb), 3), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().vt_align_resample_u8(C.c_void_p(out.data_ptr()), C.c_void_p(src.data_ptr()), src.shape[0], row0, Hs,
                                               src.shape[1], C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()),
                                               xk.shape[1], C.c_void_p(t[2].data_ptr()), C.c_void_p(t[3].data_ptr()),
                                               yk.shape[1], len(yb), len(xb), _stream(src)), "vt_align_resample_u8")
    return out


def pad_blend(base: torch.Tensor, offset: int, h0: int, w0: int, pitch: int, pad: Sequence[int], taps: np.ndarray) -> torch.Tensor:
    """vt_align_pad_blend on the (h0,w0,3) view that starts `offset` bytes into `base` with rows `pitch` bytes apart."""
    dev = base.device
    pl, pt, pr, pb = (int(p) for p in pad)
    h, w, r = h0 + pt + pb, w0 + pl + pr, len(taps) - 1
    nbytes = int(_lib.lib().vt_align_pad_blend_workspace(h, w, r))
    if nbytes <= 0:
        raise _lib.VtError(f"vt_align_pad_blend_workspace({h}, {w}, {r}): {_lib.lib().vt_last_error().decode()}")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    d_taps = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float64)).to(dev)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().vt_align_pad_blend(C.c_void_p(out.data_ptr()), C.c_void_p(base.data_ptr() + offset), h0, w0, pitch,
                                             pl, pt, pr, pb, C.c_void_p(d_taps.data_ptr()), r, C.c_void_p(ws.data_ptr()),
                                             nbytes, _stream(base)), "vt_align_pad_blend")
    return out


def quad_transform(base: torch.Tensor, offset: int, h: int, w: int, pitch: int, a: np.ndarray, size: int = OUTPUT_SIZE,
                   normalised: bool = True):
    """vt_align_quad: (size,size,3) uint8 and, when asked, (1,3,size,size) float32 = ((v / 255) - 0.5) / 0.5."""
    dev = base.device
    u8 = torch.empty((size, size, 3), dtype=torch.uint8, device=dev)
    x = torch.empty((1, 3, size, size), dtype=torch.float32, device=dev) if normalised else None
    coef = (C.c_double * 8)(*[float(v) for v in a])
    _lib.check(_lib.lib().vt_align_quad(C.c_void_p(u8.data_ptr()), C.c_void_p(x.data_ptr() if normalised else 0),
                                        C.c_void_p(base.data_ptr() + offset), h, w, pitch, coef, size, _stream(base)),
               "vt_align_quad")
    return u8, x


class FaceAligner:
    """align_face on the device: frame (H,W,3) uint8 RGB (host array or device tensor) + landmarks -> the aligned crop
    (256,256,3) uint8 and the style encoder's input (1,3,256,256) float32, both on the device.  A host frame is uploaded only
    as far as it is read: the rows of the crop box, or the rows the shrink's footprint of that box reaches."""

    def __init__(self, device):
        self.device = torch.device(device)

    def _rows(self, frame, r0: int, r1: int) -> torch.Tensor:
        if isinstance(frame, torch.Tensor):
            if frame.device != self.device:
                raise _lib.VtError(f"FaceAligner: the frame is on {frame.device}, the aligner on {self.device}")
            return frame[r0:r1].contiguous()
        return torch.from_numpy(np.array(frame[r0:r1])).to(self.device)      # (a copy: memory-mapped clips are read-only)

    def __call__(self, frame, lm):
        if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype not in (np.uint8, torch.uint8):
            raise _lib.VtError(f"FaceAligner: frame must be (H,W,3) uint8, got {tuple(frame.shape)} {frame.dtype}")
        H, W = int(frame.shape[0]), int(frame.shape[1])
        plan = align_parameters(lm, (H, W))
        if plan.shrink > 1:
            reg, xb, xk, yb, yk = _shrink_tables(plan, H, W)
            r0, r1 = int(yb[:, 0].min()), int((yb[:, 0] + yb[:, 1]).max())
            base = resample(self._rows(frame, r0, r1), r0, H, xb, xk, yb, yk)
            offset, h, w, pitch = 0, reg.y1 - reg.y0, reg.x1 - reg.x0, 3 * (reg.x1 - reg.x0)
        else:
            reg = _region(plan, W, H)
            base = self._rows(frame, reg.y0, reg.y1)
            offset, h, w, pitch = 3 * reg.x0, reg.y1 - reg.y0, reg.x1 - reg.x0, 3 * W
        if plan.pad is not None:
            if int(4.0 * plan.sigma + 0.5) > MAX_RADIUS:
                raise _lib.VtError(f"FaceAligner: blur radius {int(4.0 * plan.sigma + 0.5)} beyond {MAX_RADIUS}")
            base = pad_blend(base, offset, h, w, pitch, plan.pad, gaussian_taps(plan.sigma))
            offset, (h, w) = 0, plan.size
            pitch = 3 * w
        assert (h, w) == plan.size
        return quad_transform(base, offset, h, w, pitch, quad_coefficients(plan.quad, OUTPUT_SIZE))
