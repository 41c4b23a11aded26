"""Glue and style-path kernels one by one, through the C ABI, against float64 references at their edge shapes.

The convolutions have their own per-kernel suite (test_ops.py); the kernels around them -- BiSeNet / pSp glue
(parsing_glue.hip, norm_glue.hip), RAFT pooling and lookup (raft_corr.hip), the flow ops (flow_ops.hip) and the
batched style path (style_ops.hip) -- are called here directly through `_lib.lib().vt_*`, so that no wrapper's shape
checks limit the edges reached.  Every test runs in host emulation (CPU suite) and on the MI355X (-m gpu).

References are the reference project's operations as torch formulas on the CPU: F.max_pool2d, F.interpolate (nearest;
bilinear with both corner conventions), F.avg_pool2d, the AdaptiveAvgPool mean, F.grid_sample(align_corners=True,
zeros) with the 0.9999 mask, the window fusion of smooth_parsing_map.py, the all-pairs CorrBlock correlation sampled
bilinearly, EqualLinear, PixelNorm and the ModulatedConv2d modulation / demodulation (+ conv_transpose2d and blur).
Inputs of bf16 cases are rounded to bf16 first and the reference sees the rounded values.

Tolerances (the library and the emulation are built with -ffp-contract=off, so fp32 sequences are reproducible;
eps = 2^-23, the fp32 ulp of 1):
  * BIT-EXACT against the torch fp32 formula in the kernel's operation order: max-pool, the nearest gather with
    gate / add_vec / add, se_apply, avgpool2x2 ((((a+b)+c)+d)*0.25), eltwise2 / gru_blend, and the flow-warp MASK
    against torch fp32 grid_sample of ones.  Pixels whose float64 mask sum lies within 1e-6 of 0.9999 are left out
    of the mask comparison (the CPU's vectorised sampler may round those differently); the test asserts they are few.
  * Interpolation and lerps (resize_bilinear, upsample_bilinear_add, flow_warp values): (4 + 2 * in_size) eps of the
    largest |value| involved.  4 ulps cover the lerp roundings; the kernels compute the source coordinate in fp32 as
    aten does for fp32 tensors, which can differ from the float64 coordinate by ~2 ulps of in_size, and that shift
    moves the result by at most ulp(in_size) times the largest neighbour difference.
  * Reductions (channel_mean, corr_lookup, linear, pixel_norm, modulate): 1e-5 of the same sum taken over absolute
    values (the condition-free error bound of an fp32 sum), per element.
  * parsing_fuse: (16 + 4 * max exponent argument + 2 * max(h, w)) eps of max|parsing|: on top of the warp's
    coordinate term, expf(-mse / (2 sigma^2)) carries the fp32 error of its argument times its size.
  * bf16 outputs: half a bf16 ulp of the float64 value plus the fp32 slack above.
No loose max-rel bars.

Sentinels: every output is allocated with slack and filled with NaN (or a bit pattern); the tests assert that only
the intended elements changed -- ld padding, NHWC pad channels and the slack keep the sentinel, and gated launches
with gate 0 change nothing.

Grid-stride passes (GPU only, test_grid_stride_*): every capped launch -- grid_for (8192 blocks, norm_glue.hip), the
65536-block caps of flow_ops.hip and vt_avgpool2x2 -- gets one shape whose element count exceeds its cap.  The
avgpool case needs 1.07 GB of input (each output vector reads 64 bytes).  pg_grid's 262144-block cap
(parsing_glue.hip) would need multi-GB tensors and is left out.

COVERED at the end maps every entry point of include/vtoonify_amd.h to the tests that exercise it; a new entry point
without a test fails test_every_entry_point_has_a_test.
"""
import ast
import ctypes as C
import importlib
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from vtoonify_amd import _lib
from vtoonify_amd import kernels as K

EPS = 2.0 ** -23
SLACK = 67
F32, BF16 = torch.float32, torch.bfloat16
DT = {F32: _lib.VT_F32, BF16: _lib.VT_BF16}


# ------------------------------------------------------------------------------------------------------ helpers
def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def call(name, *args):
    """Launch an entry point.  Tensor arguments are passed as pointers and stay referenced for the call (a temporary
    device copy freed before the launch would hand its block to the next temporary)."""
    ptrs = [P(a) if isinstance(a, torch.Tensor) else a for a in args]
    _lib.check(getattr(_lib.lib(), name)(*ptrs), name)


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def rnd(g, shape, dtype=F32, scale=1.0, shift=0.0):
    """Random CPU tensor, already rounded to `dtype` (returned in that dtype)."""
    return torch.from_numpy((g.standard_normal(shape) * scale + shift).astype(np.float32)).to(dtype)


def nan_buf(n, dtype, dev):
    return torch.full((n + SLACK,), float("nan"), dtype=dtype, device=dev)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def assert_bitwise(got, want, what):
    gb, wb = bits(got), bits(want.to(got.dtype))
    assert gb.shape == wb.shape, (what, gb.shape, wb.shape)
    bad = gb != wb
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


def assert_all_nan(t, what):
    assert torch.isnan(t.detach().cpu().float()).all(), f"{what}: the sentinel was overwritten"


def bf16_half_ulp(a):
    """Half a bf16 ulp at |a| (float64)."""
    _, e = torch.frexp(a.abs())
    return torch.ldexp(torch.ones_like(a), e - 9)


def out_tol(ref, dtype, slack):
    """fp32 slack (absolute, scalar or per element), plus half a bf16 ulp of the float64 value for bf16 outputs."""
    slack = torch.as_tensor(slack, dtype=torch.float64)
    if dtype == F32:
        return slack.expand_as(ref)
    return bf16_half_ulp(ref.abs() + slack) + slack


def assert_close(got, ref, tol, what):
    g = got.detach().cpu().double()
    err = (g - ref).abs()
    bad = ~(err <= tol)          # NaN (an element never written) is bad as well
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements off, first at "
                           f"{bad.nonzero()[0].tolist()}: got {g[bad][0].item()}, want {ref[bad][0].item()}, "
                           f"max err {err[~torch.isnan(err)].max().item() if (~torch.isnan(err)).any() else 'nan'}")


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def nchw(t):
    return t.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------ vt_maxpool2d
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_maxpool2d(dev, dtype):
    g = np.random.default_rng(1)
    n = 3
    for k, s, pad in [(3, 2, 1), (2, 1, 1), (3, 1, 0), (5, 2, 2)]:
        for h, w in [(1, 1), (2, 3), (7, 5)]:
            oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
            if h + 2 * pad < k or w + 2 * pad < k:
                continue
            for c in (8, 24, 64):
                for negative in (False, True):
                    x = rnd(g, (n, h, w, c), dtype)
                    if negative:       # the -inf padding is visible only when every real value is below 0
                        x = -(x.abs() + 1).to(dtype)
                    out = nan_buf(n * oh * ow * c, dtype, dev)
                    call("vt_maxpool2d", P(out), x.to(dev), n, h, w, c, k, s, pad, DT[dtype], K._stream(out))
                    sync(dev)
                    ref = nhwc(F.max_pool2d(nchw(x.double()), k, s, pad))
                    case = f"k{k} s{s} p{pad} {h}x{w} c{c} neg={negative}"
                    assert_bitwise(out[:n * oh * ow * c].view(n, oh, ow, c), ref, case)
                    assert_all_nan(out[n * oh * ow * c:], case)
    x = torch.zeros((1, 4, 4, 16), dtype=dtype, device=dev)
    out = torch.zeros((1024,), dtype=dtype, device=dev)
    with pytest.raises(_lib.VtError):            # c % 8 != 0
        call("vt_maxpool2d", P(out), P(x), 1, 4, 4, 12, 3, 2, 1, DT[dtype], K._stream(out))
    with pytest.raises(_lib.VtError):            # 2 * pad > k
        call("vt_maxpool2d", P(out), P(x), 1, 4, 4, 16, 3, 1, 2, DT[dtype], K._stream(out))


# ------------------------------------------------------------------------------------------------ vt_gate_add_nearest
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gate_add_nearest(dev, dtype):
    g = np.random.default_rng(2)
    n, c = 2, 16
    for h, w, oh, ow in [(4, 6, 4, 6), (3, 4, 6, 8), (5, 7, 8, 3), (7, 5, 3, 8), (4, 5, 4, 10)]:
        res = rnd(g, (n, h, w, c), dtype)
        gate = rnd(g, (n, c), F32, 0.5, 1.0)           # a different gate per image
        av = rnd(g, (n, c))
        add = rnd(g, (n, h, w, c), dtype)
        for use_av in (False, True):
            for use_add in (False, True):
                out = nan_buf(n * oh * ow * c, dtype, dev)
                call("vt_gate_add_nearest", P(out), res.to(dev), gate.to(dev), av.to(dev) if use_av else None,
                     add.to(dev) if use_add else None, n, h, w, c, oh, ow, DT[dtype], K._stream(out))
                sync(dev)
                # the reference adds before up-sampling: `add` is read at the SOURCE pixel (model.py:108-121)
                t = res.float() * gate[:, None, None, :]
                if use_av:
                    t = t + av[:, None, None, :]
                if use_add:
                    t = t + add.float()
                ref = nhwc(F.interpolate(nchw(t), size=(oh, ow), mode="nearest")).to(dtype)
                case = f"{h}x{w}->{oh}x{ow} add_vec={use_av} add={use_add}"
                assert_bitwise(out[:n * oh * ow * c].view(n, oh, ow, c), ref, case)
                assert_all_nan(out[n * oh * ow * c:], case)


# ------------------------------------------------------------------------------------------------ vt_resize_bilinear
RESIZE_CASES = [  # h, w, virt_h, virt_w, step
    (4, 6, 8, 12, 1), (5, 5, 13, 13, 1), (13, 13, 5, 5, 1), (5, 13, 13, 5, 1), (1, 6, 3, 12, 1), (5, 1, 10, 4, 1),
    (4, 5, 1, 1, 1), (7, 9, 14, 18, 2), (6, 5, 13, 11, 2), (1, 1, 4, 3, 1),
]


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_resize_bilinear(dev, dtype):
    g = np.random.default_rng(3)
    n, c = 2, 3
    for h, w, vh, vw, step in RESIZE_CASES:
        x = rnd(g, (n, c, h, w))
        xd = x.to(dev)
        for align in (0, 1):
            full = F.interpolate(x.double(), size=(vh, vw), mode="bilinear", align_corners=bool(align))
            oh, ow = -(-vh // step), -(-vw // step)
            for layout, ld in ((_lib.OUT_NCHW, 0), (_lib.OUT_NHWC, c), (_lib.OUT_NHWC, 8)):
                mul = 1.0 if layout == _lib.OUT_NCHW else 0.75
                ref = full[:, :, ::step, ::step][:, :, :oh, :ow] * mul
                size = n * c * oh * ow if layout == _lib.OUT_NCHW else n * oh * ow * ld
                out = nan_buf(size, dtype, dev)
                call("vt_resize_bilinear", P(out), layout, ld, DT[dtype], P(xd), n, c, h, w, vh, vw, align, step, oh, ow,
                     mul, K._stream(out))
                sync(dev)
                if layout == _lib.OUT_NCHW:
                    got = out[:size].view(n, c, oh, ow)
                else:
                    o = out[:size].view(n, oh, ow, ld)
                    got = nchw(o[..., :c])
                    if ld > c:    # BiSeNetEngine zeroes channels 3..7 of its input once and never writes them again
                        assert_all_nan(o[..., c:], f"pad channels {h}x{w}->{vh}x{vw}")
                case = f"{h}x{w} -> {vh}x{vw} step {step} align {align} layout {layout} ld {ld}"
                assert_all_nan(out[size:], case)
                slack = (4 + 2 * max(h, w)) * EPS * float(ref.abs().max())
                assert_close(got, ref, out_tol(ref, dtype, slack), case)
    out = nan_buf(64, dtype, dev)
    with pytest.raises(_lib.VtError):   # the output grid must lie inside the virtual image
        call("vt_resize_bilinear", P(out), _lib.OUT_NCHW, 0, DT[dtype], P(torch.zeros(16, device=dev)), 1, 1, 4, 4, 8, 8,
             0, 2, 5, 4, 1.0, K._stream(out))
    with pytest.raises(_lib.VtError):   # NHWC needs ld_out >= c
        call("vt_resize_bilinear", P(out), _lib.OUT_NHWC, 2, DT[dtype], P(torch.zeros(48, device=dev)), 1, 3, 4, 4, 4, 4,
             0, 1, 4, 4, 1.0, K._stream(out))


# -------------------------------------------------------------------------------------------------- vt_channel_mean
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_channel_mean(dev, dtype):
    g = np.random.default_rng(4)
    # chunks of 64 pixels: hw = 1093 gives 18 chunks (the 16-lane chunk stride wraps) and a partial last chunk
    for n, hw, c, ld in [(2, 1093, 24, 24), (2, 1093, 24, 32), (1, 37, 8, 16), (3, 200, 40, 40)]:
        x = rnd(g, (n, hw, ld), dtype, 1.5, 0.3)
        mean = nan_buf(n * c, F32, dev)
        part = torch.zeros(K.instnorm_ws_bytes(n, hw, c), dtype=torch.uint8, device=dev)
        call("vt_channel_mean", P(mean), x.to(dev), ld, n, hw, c, P(part), DT[dtype], K._stream(mean))
        sync(dev)
        xs = x[..., :c].double()
        ref = xs.mean(dim=1)
        tol = 1e-5 * xs.abs().mean(dim=1) + 1e-30
        case = f"n{n} hw{hw} c{c} ld{ld}"
        assert_close(mean[:n * c].view(n, c), ref, tol, case)
        assert_all_nan(mean[n * c:], case)


# ------------------------------------------------------------------------------------------------------ vt_se_apply
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_se_apply(dev, dtype):
    g = np.random.default_rng(5)
    for n, oh, ow, c, sh, sw, s in [(2, 5, 7, 16, 5, 7, 1), (2, 4, 3, 24, 7, 5, 2), (1, 3, 3, 8, 5, 6, 2),
                                    (3, 1, 2, 8, 1, 3, 2)]:
        res = rnd(g, (n, oh, ow, c), dtype)
        sc = rnd(g, (n, sh, sw, c), dtype)
        gate = torch.sigmoid(rnd(g, (n, c)))
        out = nan_buf(n * oh * ow * c, dtype, dev)
        call("vt_se_apply", P(out), res.to(dev), gate.to(dev), sc.to(dev), n, oh, ow, c, sh, sw, s, DT[dtype],
             K._stream(out))
        sync(dev)
        ref = (res.float() * gate[:, None, None, :] + sc.float()[:, ::s, ::s][:, :oh, :ow]).to(dtype)  # MaxPool2d(1, s)
        case = f"{oh}x{ow} from {sh}x{sw} stride {s}"
        assert_bitwise(out[:n * oh * ow * c].view(n, oh, ow, c), ref, case)
        assert_all_nan(out[n * oh * ow * c:], case)


# ------------------------------------------------------------------------------------------ vt_upsample_bilinear_add
def _upsample_add_check(dev, dtype, g, n, h, w, H, W, c):
    x = rnd(g, (n, h, w, c), dtype)
    y = rnd(g, (n, H, W, c), dtype)
    out = nan_buf(n * H * W * c, dtype, dev)
    call("vt_upsample_bilinear_add", P(out), x.to(dev), y.to(dev), n, h, w, H, W, c, DT[dtype], K._stream(out))
    sync(dev)
    up = nhwc(F.interpolate(nchw(x.double()), size=(H, W), mode="bilinear", align_corners=True))
    ref = up + y.double()
    case = f"{h}x{w} -> {H}x{W} c{c}"
    slack = (4 + 2 * max(h, w)) * EPS * (float(x.abs().max()) + float(y.abs().max()))
    assert_close(out[:n * H * W * c].view(n, H, W, c), ref, out_tol(ref, dtype, slack), case)
    assert_all_nan(out[n * H * W * c:], case)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_upsample_bilinear_add(dev, dtype):
    g = np.random.default_rng(6)
    for h, w, H, W in [(16, 16, 32, 32), (32, 32, 64, 64), (5, 13, 13, 5), (13, 5, 5, 13), (1, 4, 3, 8), (4, 5, 1, 3)]:
        _upsample_add_check(dev, dtype, g, 2, h, w, H, W, 8 if H * W > 1024 else 16)


# ---------------------------------------------------------------------------------------------------- vt_avgpool2x2
def test_avgpool2x2(dev):
    g = np.random.default_rng(7)
    for n, h, w, c in [(2, 5, 7, 4), (1, 6, 4, 128), (3, 3, 3, 8), (1, 2, 2, 4)]:
        x = rnd(g, (n, h, w, c))
        oh, ow = h // 2, w // 2
        out = nan_buf(n * oh * ow * c, F32, dev)
        call("vt_avgpool2x2", P(out), x.to(dev), n, h, w, c, K._stream(out))
        sync(dev)
        got = out[:n * oh * ow * c].view(n, oh, ow, c)
        a, b = x[:, 0:2 * oh:2, 0:2 * ow:2], x[:, 0:2 * oh:2, 1:2 * ow:2]
        cc, d = x[:, 1:2 * oh:2, 0:2 * ow:2], x[:, 1:2 * oh:2, 1:2 * ow:2]
        case = f"{n}x{h}x{w}x{c}"
        assert_bitwise(got, (((a + b) + cc) + d) * 0.25, case)            # the kernel's order, in fp32
        ref = nhwc(F.avg_pool2d(nchw(x.double()), 2, stride=2))          # floor on odd sizes
        assert_close(got, ref, 2 * EPS * float(ref.abs().max()) + 4 * EPS * ref.abs(), case)
        assert_all_nan(out[n * oh * ow * c:], case)
    out = nan_buf(64, F32, dev)
    for h, w, c in [(1, 4, 4), (4, 1, 4), (4, 4, 6)]:
        with pytest.raises(_lib.VtError):
            call("vt_avgpool2x2", P(out), P(torch.zeros(64, device=dev)), 1, h, w, c, K._stream(out))


# --------------------------------------------------------------------------------------------------- vt_corr_lookup
def _bilerp_zero(vol, X, Y):
    """vol (P,H,W) float64, X/Y (P,K) float64 -> (P,K): bilinear, zero outside (grid_sample align_corners=True)."""
    Pn, H, W = vol.shape
    flat = vol.reshape(Pn, H * W)
    x0, y0 = torch.floor(X), torch.floor(Y)
    fx, fy = X - x0, Y - y0
    out = torch.zeros_like(X)
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = x0 + dx, y0 + dy
            inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
            out = out + torch.where(inside, torch.gather(flat, 1, idx) * wx * wy, torch.zeros_like(X))
    return out


def corr_reference(f1, f2, coords, r, scale, coord_scale):
    """All-pairs correlation (CorrBlock, corr.py:12-60) sampled bilinearly around coords * coord_scale, float64;
    also the same sum over absolute values (the error bound)."""
    B, H1, W1, Cc = f1.shape
    H2, W2 = f2.shape[1:3]
    rd = 2 * r + 1
    xy = (coords.float() * coord_scale).double().reshape(B * H1 * W1, 2)      # the kernel scales in fp32 (exact)
    off = torch.arange(-r, r + 1, dtype=torch.float64)
    oa, ob = torch.meshgrid(off, off, indexing="ij")                         # output channel a + rd * b: a = y offset
    X = xy[:, :1] + ob.T.reshape(1, -1)
    Y = xy[:, 1:] + oa.T.reshape(1, -1)
    outs = []
    for absval in (False, True):
        a1, a2 = (f1.double().abs(), f2.double().abs()) if absval else (f1.double(), f2.double())
        vol = torch.einsum("bpc,bqc->bpq", a1.reshape(B, H1 * W1, Cc), a2.reshape(B, H2 * W2, Cc))
        v = _bilerp_zero(vol.reshape(B * H1 * W1, H2, W2), X, Y)
        outs.append(v.reshape(B, H1 * W1, rd * rd).permute(0, 2, 1).reshape(B, 1, rd * rd, H1, W1) * abs(scale))
    outs[0] = outs[0] * math.copysign(1.0, scale)
    return outs


def _corr_coords(g, B, H1, W1, H2, W2, coord_scale):
    """Target coordinates (in the level's pixels) of every kind, then divided by coord_scale (exact: powers of 2)."""
    npx = B * H1 * W1
    kinds = np.arange(npx) % 5
    x = g.uniform(-2, W2 + 1, npx)
    y = g.uniform(-2, H2 + 1, npx)
    on = kinds == 0                       # integer grid points
    x[on], y[on] = np.round(x[on]), np.round(y[on])
    last = kinds == 1                     # fractional, inside the last row and column
    x[last], y[last] = W2 - 1 + g.uniform(0.05, 0.95, last.sum()), H2 - 1 + g.uniform(0.05, 0.95, last.sum())
    far = kinds == 2                      # far outside
    x[far], y[far] = np.where(g.random(far.sum()) < 0.5, 1e4, -1e4), g.uniform(0, H2, far.sum())
    xy = np.stack([x, y], -1).astype(np.float32) / np.float32(coord_scale)
    return torch.from_numpy(xy).reshape(B, 1, H1, W1, 2)


def test_corr_lookup(dev):
    g = np.random.default_rng(8)
    cases = [  # r, C, B, H1, W1, H2, W2, scale, coord_scale   (B*H1*W1 never a multiple of CORR_WAVES = 4)
        (0, 4, 1, 3, 3, 4, 5, 1.0, 1.0), (1, 36, 3, 1, 5, 6, 4, 0.5, 0.5), (4, 36, 1, 5, 3, 7, 9, -0.25, 0.25),
        (8, 4, 1, 3, 5, 9, 11, 1.0, 1.0), (8, 512, 1, 1, 7, 5, 6, 1 / math.sqrt(512), 0.5), (1, 512, 1, 3, 3, 4, 4, 1.0, 1.0),
        (4, 4, 2, 3, 3, 2, 3, 1.0, 0.25),
    ]
    for r, Cc, B, H1, W1, H2, W2, scale, cs in cases:
        f1, f2 = rnd(g, (B, H1, W1, Cc)), rnd(g, (B, H2, W2, Cc))
        coords = _corr_coords(g, B, H1, W1, H2, W2, cs)
        rd = 2 * r + 1
        size = B * rd * rd * H1 * W1
        out = nan_buf(size, F32, dev)
        call("vt_corr_lookup", P(out), f1.to(dev), f2.to(dev), coords.to(dev), B, H1, W1, H2, W2, Cc, r, scale,
             cs, K._stream(out))
        sync(dev)
        ref, bound = corr_reference(f1, f2, coords, r, scale, cs)
        case = f"r{r} C{Cc} {B}x{H1}x{W1} -> {H2}x{W2} scale {scale} coord_scale {cs}"
        assert_close(out[:size].view(B, 1, rd * rd, H1, W1), ref, 1e-5 * bound + 1e-30, case)
        assert_all_nan(out[size:], case)
    out = nan_buf(1024, F32, dev)
    z = torch.zeros(4096, device=dev)
    for Cc, r in [(516, 1), (36, 9), (6, 1)]:
        with pytest.raises(_lib.VtError):
            call("vt_corr_lookup", P(out), P(z), P(z), P(z), 1, 1, 1, 2, 2, Cc, r, 1.0, 1.0, K._stream(out))


# ----------------------------------------------------------------------------------------------------- vt_flow_warp
def _vgrid(flo):
    """smooth_parsing_map.py:45-59 in fp32 (the reference's dtype): normalised sampling grid (B,H,W,2)."""
    B, _, H, W = flo.shape
    xx = torch.arange(W, dtype=F32).view(1, 1, W).expand(B, H, W)
    yy = torch.arange(H, dtype=F32).view(1, H, 1).expand(B, H, W)
    vx = 2.0 * (xx + flo[:, 0]) / max(W - 1, 1) - 1.0
    vy = 2.0 * (yy + flo[:, 1]) / max(H - 1, 1) - 1.0
    return torch.stack([vx, vy], -1)


def warp_reference(x, flo):
    """-> (mask32, keep, sample64): the torch fp32 mask (grid_sample of ones, < 0.9999 -> 0), the pixels whose float64
    mask sum is not within 1e-6 of the threshold, and the float64 grid_sample of x on the same fp32 grid."""
    B, Cc, H, W = x.shape
    grid = _vgrid(flo)
    ones = torch.ones((B, 1, H, W), dtype=F32)
    m32 = F.grid_sample(ones, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
    m64 = F.grid_sample(ones.double(), grid.double(), mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
    mask = (m32 >= 0.9999).to(F32)
    keep = (m64 - 0.9999).abs() > 1e-6
    sample = F.grid_sample(x.double(), grid.double(), mode="bilinear", padding_mode="zeros", align_corners=True)
    return mask, keep, sample


def _flows(g, B, H, W):
    """Every kind of flow, pixel by pixel: fractional, integer (zero-weight corners), landing exactly on the last row /
    column, +-1e4 (the corner clamp), and a small fraction of a pixel outside the border (mask sums in (0.999, 0.9999))."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx, fy = g.uniform(-3, 3, (B, H, W)), g.uniform(-3, 3, (B, H, W))
    kind = (np.arange(B * H * W).reshape(B, H, W) * 7 + 3) % 6
    ints = kind == 0
    fx[ints], fy[ints] = np.round(fx[ints]), np.round(fy[ints])
    last = kind == 1
    fx[last] = ((W - 1) - xx)[None].repeat(B, 0)[last]
    fy[last] = ((H - 1) - yy)[None].repeat(B, 0)[last]
    far = kind == 2
    fx[far] = np.where(g.random(far.sum()) < 0.5, 1e4, -1e4)
    eps = g.choice([2e-4, 5e-4, 8e-4, 2e-3], (B, H, W))
    left, right = kind == 3, kind == 4
    fx[left] = (-xx[None] - eps)[left]                    # just left of column 0
    fx[right] = ((W - 1) - xx[None] + eps)[right]         # just right of the last column
    fy[left | right] = np.round(fy[left | right]).clip(-yy[None].repeat(B, 0)[left | right],
                                                       (H - 1 - yy)[None].repeat(B, 0)[left | right])
    top = (kind == 5) & (g.random((B, H, W)) < 0.5)
    fy[top] = (-yy[None] - eps)[top]
    return torch.from_numpy(np.stack([fx, fy], 1).astype(np.float32))


def _warp_check(dev, B, Cc, H, W, g, with_mask=True, min_between=0):
    x = rnd(g, (B, Cc, H, W))
    flo = _flows(g, B, H, W)
    out = nan_buf(B * Cc * H * W, F32, dev)
    mask = nan_buf(B * H * W, F32, dev)
    call("vt_flow_warp", P(out), P(mask) if with_mask else P(None), x.to(dev), flo.to(dev), B, Cc, H, W,
         K._stream(out))
    sync(dev)
    m_ref, keep, sample = warp_reference(x, flo)
    case = f"{B}x{Cc}x{H}x{W}"
    assert int((~keep).sum()) <= max(2, keep.numel() // 100), f"{case}: {int((~keep).sum())} pixels at the threshold"
    if with_mask:
        got_m = mask[:B * H * W].view(B, H, W)
        assert_bitwise(got_m[keep], m_ref[keep], case + " mask")
        assert_all_nan(mask[B * H * W:], case + " mask slack")
    else:
        assert_all_nan(mask, case + " mask untouched")
    ref = sample * m_ref[:, None]
    keepc = keep[:, None].expand(B, Cc, H, W)
    got = out[:B * Cc * H * W].view(B, Cc, H, W)
    slack = (4 + 2 * max(H, W)) * EPS * float(x.abs().max())
    assert_close(got[keepc], ref[keepc], slack, case)
    zero = (m_ref[:, None].expand(B, Cc, H, W) == 0) & keepc
    assert bool((got.cpu()[zero] == 0).all()), f"{case}: masked pixels must be exactly 0"
    assert_all_nan(out[B * Cc * H * W:], case)
    # the threshold matters: some pixels have mask sums in (0.999, 0.9999) and must be 0
    m64 = F.grid_sample(torch.ones((B, 1, H, W), dtype=torch.float64), _vgrid(flo).double(), align_corners=True)[:, 0]
    between = (m64 > 0.999) & (m64 < 0.9999 - 1e-6)
    assert int(between.sum()) >= min_between, case
    return between


def test_flow_warp(dev):
    g = np.random.default_rng(9)
    between = 0
    for B, Cc, H, W in [(2, 3, 9, 14), (1, 22, 7, 5), (2, 1, 6, 1), (1, 3, 1, 7), (1, 22, 1, 1), (3, 1, 11, 13)]:
        between += int(_warp_check(dev, B, Cc, H, W, g).sum())
    assert between >= 10       # the 0.9999 threshold (not 0.999) is exercised
    _warp_check(dev, 1, 2, 5, 6, g, with_mask=False)          # mask == NULL


# -------------------------------------------------------------------------------------------------- vt_parsing_fuse
def fuse_reference(image1, image2, parsing, flow, wt, ci, sigma):
    """smooth_parsing_map.py:155-166 in float64 on the fp32 grid, with the fp32 mask; -> (fused, keep, max exp arg)."""
    wn, cp, H, W = parsing.shape
    x = torch.cat([image2, parsing], 1)
    mask, keep, sample = warp_reference(x, flow)
    aI, aP = sample[:, :3], sample[:, 3:].clone()
    arg = ((aI - image1.double()[None]) ** 2).mean(dim=1) / (2 * sigma ** 2)
    ws = torch.exp(-arg) * mask.double()
    aP[ci] = parsing[ci].double()
    ws[ci] = 1.0
    keep[ci] = True
    wts = ws * wt.double().view(-1, 1, 1)
    fused = (aP * (wts / wts.sum(0, keepdim=True))[:, None]).sum(0)
    arg[ci] = 0
    return fused, keep.all(0), float((arg * mask.double()).max())


def test_parsing_fuse(dev):
    g = np.random.default_rng(10)
    H, W = 5, 7
    for wn, cis in [(1, [0]), (3, [0, 1, 2]), (5, [0, 2, 4])]:
        for ci in cis:
            for cp, sigma in [(1, 0.2), (19, 0.5), (32, 1.3)]:
                image1 = rnd(g, (3, H, W), F32, 0.5)
                image2 = (image1[None] + rnd(g, (wn, 3, H, W), F32, 0.3)).contiguous()
                parsing = torch.softmax(rnd(g, (wn, cp, H, W), F32, 2.0), 1).contiguous()
                flow = _flows(g, wn, H, W)
                wt = torch.exp(-(torch.arange(wn, dtype=F32) - ci) ** 2 / 4.5) + 0.1
                out = nan_buf(cp * H * W, F32, dev)
                call("vt_parsing_fuse", P(out), image2.to(dev), image1.to(dev), parsing.to(dev), flow.to(dev),
                     wt.to(dev), wn, ci, cp, H, W, sigma, K._stream(out))
                sync(dev)
                ref, keep, argmax = fuse_reference(image1, image2, parsing, flow, wt, ci, sigma)
                case = f"wn{wn} ci{ci} cp{cp} sigma{sigma}"
                assert int((~keep).sum()) <= 2, case
                slack = (16 + 4 * argmax + 2 * max(H, W)) * EPS * float(parsing.abs().max())
                got = out[:cp * H * W].view(cp, H, W)
                assert_close(got[:, keep], ref[:, keep], slack, case)
                assert_all_nan(out[cp * H * W:], case)
    # a window whose neighbours are all masked out: the centre map, to within 1 ulp
    wn, ci, cp = 5, 2, 19
    image1 = rnd(g, (3, H, W))
    image2 = rnd(g, (wn, 3, H, W))
    parsing = torch.softmax(rnd(g, (wn, cp, H, W)), 1).contiguous()
    flow = torch.full((wn, 2, H, W), 1e4)
    wt = torch.tensor([0.3, 0.7, 0.9, 0.7, 0.3])
    out = nan_buf(cp * H * W, F32, dev)
    call("vt_parsing_fuse", P(out), image2.to(dev), image1.to(dev), parsing.to(dev), flow.to(dev), wt.to(dev),
         wn, ci, cp, H, W, 0.2, K._stream(out))
    sync(dev)
    c = parsing[ci].double()
    assert_close(out[:cp * H * W].view(cp, H, W), c, EPS * c.abs(), "all neighbours masked")
    with pytest.raises(_lib.VtError):     # at most 32 classes in registers
        call("vt_parsing_fuse", P(out), image2.to(dev), image1.to(dev), P(out), flow.to(dev), wt.to(dev),
             1, 0, 33, 1, 1, 0.2, K._stream(out))
    with pytest.raises(_lib.VtError):     # the centre frame must be inside the window
        call("vt_parsing_fuse", P(out), image2.to(dev), image1.to(dev), parsing.to(dev), flow.to(dev),
             wt.to(dev), wn, wn, cp, H, W, 0.2, K._stream(out))


# ------------------------------------------------------------------------------------- vt_linear_batch[_gated]
ACTS = (_lib.ACT_NONE, _lib.ACT_LRELU, _lib.ACT_SIGMOID)


def _linear_items(g, n_items=30):
    """Item specs: quad and non-quad in_dim, row tails, ld padding, b NULL or not, all three acts."""
    specs = []
    for i in range(n_items):
        in_dim = (7, 22, 512, 8, 64)[i % 5]
        rows = (1, 5, 6, 7, 18)[(i // 2) % 5]
        out_dim = 1 + (i * 7) % 9
        ld_x = in_dim + (0, 4, 3)[i % 3]
        ld_y = out_dim + (0, 2)[(i // 3) % 2]
        spec = dict(in_dim=in_dim, rows=rows, out_dim=out_dim, ld_x=ld_x, ld_y=ld_y, act=ACTS[i % 3],
                    w_scale=float(g.uniform(0.05, 0.5)), b_scale=float(g.uniform(0.5, 2)), slope=0.2, gain=2 ** 0.5,
                    x=rnd(g, (rows, ld_x)), W=rnd(g, (out_dim, in_dim)),
                    b=rnd(g, (out_dim,)) if i % 4 != 1 else None)
        specs.append(spec)
    return specs


def _linear_run(dev, specs, offset=False, gate=None, ys=None):
    """Launch all items in one vt_linear_batch[_gated] call.  offset=True: W and x are 4-byte-offset views."""
    keep, items = [], []
    for i, s in enumerate(specs):
        if offset:
            wb = torch.zeros(s["W"].numel() + 8, device=dev)
            Wd = wb[1:1 + s["W"].numel()]
            Wd.copy_(s["W"].reshape(-1).to(dev))
            xb = torch.zeros(s["x"].numel() + 8, device=dev)
            xd = xb[1:1 + s["x"].numel()]
            xd.copy_(s["x"].reshape(-1).to(dev))
            assert Wd.data_ptr() % 16 == 4 and xd.data_ptr() % 16 == 4
        else:
            Wd, xd = s["W"].to(dev), s["x"].to(dev)
            assert Wd.data_ptr() % 16 == 0 and xd.data_ptr() % 16 == 0
        bd = s["b"].to(dev) if s["b"] is not None else None
        y = ys[i] if ys is not None else nan_buf(s["rows"] * s["ld_y"], F32, dev)
        keep += [Wd, xd, bd, y]
        items.append(_lib.LinearItem(y.data_ptr(), xd.data_ptr(), Wd.data_ptr(), 0 if bd is None else bd.data_ptr(),
                                     s["ld_y"], s["ld_x"], s["rows"], s["in_dim"], s["out_dim"], s["act"], s["w_scale"],
                                     s["b_scale"], s["slope"], s["gain"]))
    arr = (_lib.LinearItem * len(items))(*items)
    st = K._stream(keep[0])
    if gate is None:
        call("vt_linear_batch", arr, len(items), st)
    else:
        call("vt_linear_batch_gated", arr, len(items), P(gate), st)
    sync(dev)
    return [keep[4 * i + 3] for i in range(len(specs))]


def _linear_ref(s):
    x = s["x"][:, :s["in_dim"]].double()
    Wt = s["W"].double().T
    v = x @ Wt * s["w_scale"]
    bound = x.abs() @ Wt.abs() * abs(s["w_scale"])
    if s["b"] is not None:
        v = v + s["b"].double() * s["b_scale"]
        bound = bound + (s["b"].double() * s["b_scale"]).abs()
    if s["act"] == _lib.ACT_LRELU:
        v, bound = torch.where(v > 0, v, v * s["slope"]) * s["gain"], bound * s["gain"]
    elif s["act"] == _lib.ACT_SIGMOID:
        v, bound = torch.sigmoid(v), bound * 0.25
    return v, 1e-5 * bound + 4 * EPS * v.abs() + 1e-30


def test_linear_batch(dev):
    g = np.random.default_rng(11)
    specs = _linear_items(g)                                   # 30 items: two launches of <= 24
    ys = _linear_run(dev, specs)
    for i, (s, y) in enumerate(zip(specs, ys)):
        n = s["rows"] * s["ld_y"]
        yy = y[:n].view(s["rows"], s["ld_y"])
        ref, tol = _linear_ref(s)
        case = f"item {i}: rows {s['rows']} in {s['in_dim']} out {s['out_dim']} ld_x {s['ld_x']} act {s['act']}"
        assert_close(yy[:, :s["out_dim"]], ref, tol, case)
        assert_all_nan(yy[:, s["out_dim"]:], case + " ld_y padding")
        assert_all_nan(y[n:], case + " slack")
    # the summation order depends on the shape only: 4-byte-offset views give the bits of 16-byte-aligned tensors
    ys_off = _linear_run(dev, specs, offset=True)
    for i, (a, b) in enumerate(zip(ys, ys_off)):
        assert_bitwise(b, a, f"item {i}: offset views")
    # gated: gate 0 changes nothing, gate 1 is the ungated launch bit for bit
    gate = torch.tensor([0, 0], dtype=torch.int32, device=dev)
    pre = [nan_buf(s["rows"] * s["ld_y"], F32, dev) for s in specs]
    for y in pre:
        y[: y.numel() // 2] = 3.0
    snap = [y.clone() for y in pre]
    _linear_run(dev, specs, gate=gate, ys=pre)
    for i, (a, b) in enumerate(zip(pre, snap)):
        assert_bitwise(a, b, f"item {i}: gate 0")
    gate.fill_(1)
    ys_g = _linear_run(dev, specs, gate=gate)
    for i, (a, b) in enumerate(zip(ys_g, ys)):
        assert_bitwise(a, b, f"item {i}: gate 1")


# ------------------------------------------------------------------------------- vt_modulate_weight_batch[_gated]
BLUR = (np.outer([1, 3, 3, 1], [1, 3, 3, 1]) / 64.0 * 4.0).astype(np.float32)   # make_kernel([1,3,3,1]) * 2^2


def _mod_items(g, n_items=20):
    specs = []
    for i in range(n_items):
        k = (3, 1)[i % 2] if i % 5 != 4 else 3
        fir = (i % 4 == 0) and k == 3
        cin = (3, 17, 70, 64, 300)[i % 5]
        cout = 1 + (i * 3) % 4
        specs.append(dict(k=k, cin=cin, cout=cout, demod=int(i % 3 != 2), fir=fir,
                          scale=1.0 / math.sqrt(cin * k * k), w=rnd(g, (cout, cin, k, k)), s=rnd(g, (cin,), F32, 0.5, 1.0)))
    return specs


def _mod_size(s):
    return 4 * s["cout"] * 9 * s["cin"] if s["fir"] else s["cout"] * s["k"] ** 2 * s["cin"]


def _mod_run(dev, specs, dtype, gate=None, outs=None):
    keep, items = [], []
    fir = torch.from_numpy(BLUR).to(dev)
    for i, s in enumerate(specs):
        out = outs[i] if outs is not None else nan_buf(_mod_size(s), dtype, dev)
        w, sv = s["w"].to(dev), s["s"].to(dev)
        keep += [out, w, sv]
        items.append(_lib.ModulateItem(out.data_ptr(), w.data_ptr(), sv.data_ptr(), fir.data_ptr() if s["fir"] else 0,
                                       s["cout"], s["cin"], s["k"], s["demod"], s["scale"], 0))
    arr = (_lib.ModulateItem * len(items))(*items)
    if gate is None:
        call("vt_modulate_weight_batch", arr, len(items), DT[dtype], K._stream(fir))
    else:
        call("vt_modulate_weight_batch_gated", arr, len(items), DT[dtype], P(gate), K._stream(fir))
    sync(dev)
    return [keep[3 * i] for i in range(len(specs))]


def _modulated(s):
    """model.py:259-267 in float64: w' = scale * w * s, demodulated -> (cout, cin, k, k)."""
    w = s["w"].double() * s["scale"] * s["s"].double().view(1, -1, 1, 1)
    if s["demod"]:
        w = w * torch.rsqrt((w ** 2).sum((1, 2, 3), keepdim=True) + 1e-8)
    return w


def _polyphase_apply(weff, x, cout):
    """The four 3x3 polyphase filters [4*cout][9][cin] applied by gather: out[co, 2Y+py, 2X+px] =
    sum_{ky,kx,ci} weff[p*cout+co][ky*3+kx][ci] * x[ci, Y+ky-1, X+kx-1] (zero outside)."""
    cin, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros((cout, 2 * H, 2 * W), dtype=torch.float64)
    wr = weff.view(4, cout, 3, 3, cin)
    for p in range(4):
        py, px = p >> 1, p & 1
        acc = torch.zeros((cout, H, W), dtype=torch.float64)
        for ky in range(3):
            for kx in range(3):
                acc += torch.einsum("oc,chw->ohw", wr[p, :, ky, kx], xp[:, ky:ky + H, kx:kx + W])
        out[:, py::2, px::2] = acc
    return out


def _convT_blur(wmod, x):
    """conv_transpose2d(stride 2) then Blur(pad (1,1)) = upfirdn2d with the flipped 4x4 FIR (model.py:273-286)."""
    cout = wmod.shape[0]
    y = F.conv_transpose2d(x[None], wmod.transpose(0, 1), stride=2)[0]            # (cout, 2H+1, 2W+1)
    k = torch.from_numpy(BLUR).double().flip(0, 1)
    return F.conv2d(F.pad(y, (1, 1, 1, 1))[:, None], k[None, None])[:, 0]         # (cout, 2H, 2W)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_modulate_weight_batch(dev, dtype):
    g = np.random.default_rng(12)
    specs = _mod_items(g)                                     # 20 items: two launches of <= 16
    outs = _mod_run(dev, specs, dtype)
    for i, (s, out) in enumerate(zip(specs, outs)):
        n = _mod_size(s)
        case = f"item {i}: cout {s['cout']} cin {s['cin']} k {s['k']} demod {s['demod']} fir {s['fir']}"
        assert_all_nan(out[n:], case + " slack")
        got = out[:n].cpu()
        wm = _modulated(s)
        if not s["fir"]:
            ref = wm.permute(0, 2, 3, 1).reshape(s["cout"], s["k"] ** 2, s["cin"])   # packed [co][tap][ci]
            assert_close(got.view_as(ref), ref, out_tol(ref, dtype, 1e-5 * ref.abs() + 1e-30), case)
        else:
            x = rnd(g, (s["cin"], 4, 5)).double()
            ref = _convT_blur(wm, x)
            weff = got.double()
            y = _polyphase_apply(weff, x, s["cout"])
            bound = _polyphase_apply(weff.abs(), x.abs(), s["cout"])
            rel = 2e-5 if dtype == F32 else 2e-5 + 2.0 ** -8
            assert_close(y, ref, rel * bound + 1e-30, case + " (conv_transpose2d + blur)")
        # the single-item kernel (one wavefront per channel, another reduction order) agrees to fp32 tolerance
        single = nan_buf(n, dtype, dev)
        fir = torch.from_numpy(BLUR).to(dev) if s["fir"] else None
        call("vt_modulate_weight", P(single), s["w"].to(dev), s["s"].to(dev), s["cout"], s["cin"], s["k"],
             s["scale"], s["demod"], P(fir), DT[dtype], K._stream(single))
        sync(dev)
        a, b = single[:n].cpu().double(), got.double()
        # (the polyphase taps are sums of up to four products: a few ulps of the item's largest tap on top)
        slack = 1e-5 * b.abs() + 8 * EPS * float(b.abs().max())
        assert_close(a, b, out_tol(b, dtype, slack) * (2 if dtype == BF16 else 1), case + " vs single")
        assert_all_nan(single[n:], case + " single slack")
    gate = torch.tensor([0, 0], dtype=torch.int32, device=dev)
    pre = [torch.full((_mod_size(s) + SLACK,), 5.0, dtype=dtype, device=dev) for s in specs]
    snap = [t.clone() for t in pre]
    _mod_run(dev, specs, dtype, gate=gate, outs=pre)
    for i, (a, b) in enumerate(zip(pre, snap)):
        assert_bitwise(a, b, f"item {i}: gate 0")
    gate.fill_(1)
    for i, (a, b) in enumerate(zip(_mod_run(dev, specs, dtype, gate=gate), outs)):
        assert_bitwise(a, b, f"item {i}: gate 1")


# -------------------------------------------------------------------------------------------- vt_pixel_norm[_gated]
def test_pixel_norm(dev):
    g = np.random.default_rng(13)
    for rows in (1, 5, 18):
        for dim in (7, 512):
            x = rnd(g, (rows, dim), F32, 2.0)
            y = nan_buf(rows * dim, F32, dev)
            call("vt_pixel_norm", P(y), x.to(dev), rows, dim, K._stream(y))
            sync(dev)
            xd = x.double()
            ref = xd * torch.rsqrt((xd ** 2).mean(1, keepdim=True) + 1e-8)          # model.py:17-18
            case = f"rows {rows} dim {dim}"
            assert_close(y[:rows * dim].view(rows, dim), ref, 1e-5 * ref.abs() + 1e-30, case)
            assert_all_nan(y[rows * dim:], case)
            gate = torch.tensor([0, 0], dtype=torch.int32, device=dev)
            y0 = nan_buf(rows * dim, F32, dev)
            call("vt_pixel_norm_gated", P(y0), x.to(dev), rows, dim, P(gate), K._stream(y0))
            sync(dev)
            assert_all_nan(y0, case + " gate 0")
            gate.fill_(1)
            call("vt_pixel_norm_gated", P(y0), x.to(dev), rows, dim, P(gate), K._stream(y0))
            sync(dev)
            assert_bitwise(y0, y, case + " gate 1")


# ---------------------------------------------------------------------------------------------------- vt_style_gate
def test_style_gate(dev):
    g = np.random.default_rng(14)
    for n in (1, 255, 256, 9217):
        base = rnd(g, (n,))

        def run(cached_vals, fresh_vals, flag_in):
            cached = torch.full((n + SLACK,), -7.0, device=dev)
            cached[:n] = cached_vals.to(dev)
            fresh = fresh_vals.to(dev).contiguous()
            flag = torch.tensor(flag_in, dtype=torch.int32, device=dev)
            call("vt_style_gate", P(flag), P(cached), P(fresh), n, K._stream(flag))
            sync(dev)
            assert bool((cached[n:].cpu() == -7.0).all()), f"n {n}: cached slack overwritten"
            return flag.cpu().tolist(), cached[:n]

        flag, cached = run(base, base.clone(), [7, 0])
        assert flag == [0, 0], n
        assert_bitwise(cached, base, f"n {n}: unchanged")
        for idx in sorted({0, n // 2, n - 1}):
            fresh = base.clone()
            fresh[idx] += 1.0
            flag, cached = run(base, fresh, [0, 0])
            assert flag == [1, 0], (n, idx)
            assert_bitwise(cached, fresh, f"n {n}: adopted after a change at {idx}")
        # bitwise: -0.0 against 0.0 and another NaN payload are changes
        c0, f0 = base.clone(), base.clone()
        c0[n - 1], f0[n - 1] = 0.0, -0.0
        flag, cached = run(c0, f0, [0, 0])
        assert flag == [1, 0], (n, "-0.0")
        assert_bitwise(cached, f0, f"n {n}: -0.0 adopted")
        c1, f1 = base.clone(), base.clone()
        c1.view(torch.int32)[0] = 0x7FC00000
        f1.view(torch.int32)[0] = 0x7FC00001
        flag, cached = run(c1, f1, [0, 0])
        assert flag == [1, 0], (n, "NaN payload")
        assert_bitwise(cached, f1, f"n {n}: NaN payload adopted")
        # the force word: flag 1 on identical rows, and the force word is cleared
        flag, cached = run(base, base.clone(), [0, 1])
        assert flag == [1, 0], (n, "force")
        assert_bitwise(cached, base, f"n {n}: forced")


# ------------------------------------------------------------------------------------- grid-stride passes (GPU only)
@pytest.mark.gpu
def test_grid_stride_upsample_bilinear_add(dev):
    """2 x 256^2 x 256 bf16: 4.2 M vectors, twice grid_for's 8192 x 256."""
    if dev.type != "cuda":
        pytest.skip("GPU-only shape")
    _upsample_add_check(dev, BF16, np.random.default_rng(20), 2, 128, 128, 256, 256, 256)


@pytest.mark.gpu
def test_grid_stride_flow_warp(dev):
    """1 x 1 x 4104 x 4104: 16.84 M pixels, more than the 65536 x 256 cap of flow_ops.hip."""
    if dev.type != "cuda":
        pytest.skip("GPU-only shape")
    _warp_check(dev, 1, 1, 4104, 4104, np.random.default_rng(21), min_between=1)


@pytest.mark.gpu
def test_grid_stride_avgpool2x2(dev):
    """4 x 4098 x 4098 x 4: 16.79 M output vectors, more than the 65536 x 256 cap of vt_avgpool2x2."""
    if dev.type != "cuda":
        pytest.skip("GPU-only shape")
    n, h, w, c = 4, 4098, 4098, 4
    gen = torch.Generator(device=dev).manual_seed(22)
    x = torch.randn((n, h, w, c), device=dev, generator=gen)
    oh, ow = h // 2, w // 2
    out = nan_buf(n * oh * ow * c, F32, dev)
    call("vt_avgpool2x2", P(out), P(x), n, h, w, c, K._stream(out))
    sync(dev)
    # element-wise fp32 adds and a multiply, one kernel each: correctly rounded on any device
    a, b = x[:, 0::2, 0::2], x[:, 0::2, 1::2]
    cc, d = x[:, 1::2, 0::2], x[:, 1::2, 1::2]
    want = (((a + b) + cc) + d) * 0.25
    got = out[:n * oh * ow * c].view(n, oh, ow, c)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool(torch.isnan(out[n * oh * ow * c:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_grid_stride_eltwise2_gru_blend(dev, dtype):
    """rows * c = 16.78 M + 48 elements, more than the 65536 x 256 cap of flow_ops.hip; row strides with padding."""
    if dev.type != "cuda":
        pytest.skip("GPU-only shape")
    rows, c, ld = (1 << 20) + 3, 16, 24
    gen = torch.Generator().manual_seed(23)
    a = torch.randn((rows, ld), generator=gen).to(dtype)
    b = torch.randn((rows, ld), generator=gen).to(dtype)
    ad, bd = a.to(dev), b.to(dev)
    for op in (0, 1, 2):
        out = nan_buf(rows * ld, dtype, dev)
        call("vt_eltwise2", P(out), ld, P(ad), ld, P(bd), ld, rows, c, op, DT[dtype], K._stream(out))
        sync(dev)
        af, bf = a[:, :c].float(), b[:, :c].float()
        want = af * bf if op == 0 else (af + bf if op == 1 else torch.relu(af + bf))
        o = out[:rows * ld].view(rows, ld).cpu()
        assert_bitwise(o[:, :c], want.to(dtype), f"eltwise2 op {op}")
        assert_all_nan(o[:, c:], f"eltwise2 op {op} padding")
        assert_all_nan(out[rows * ld:], f"eltwise2 op {op} slack")
    z = torch.rand((rows, c), generator=gen).to(dtype)
    q = torch.randn((rows, c), generator=gen).to(dtype)
    h = nan_buf(rows * ld, dtype, dev)
    h[:rows * ld].view(rows, ld)[:, :c] = a[:, :c].to(dev)
    call("vt_gru_blend", P(h), ld, z.to(dev), q.to(dev), rows, c, DT[dtype], K._stream(h))
    sync(dev)
    zf, hf, qf = z.float(), a[:, :c].float(), q.float()
    o = h[:rows * ld].view(rows, ld).cpu()
    assert_bitwise(o[:, :c], ((1.0 - zf) * hf + zf * qf).to(dtype), "gru_blend")
    assert_all_nan(o[:, c:], "gru_blend padding")
    assert_all_nan(h[rows * ld:], "gru_blend slack")


# --------------------------------------------------------------------------------------------- ABI coverage guard
# entry point -> (tests that exercise it, wrapper chain or None).  With a wrapper chain ("kernels.linear", ...), the
# tests call the first wrapper, every wrapper's source names the next one, and the last one names the entry point.
GLUE = "test_glue_ops"
NORM = "test_norm_native_ops"
COVERED = {
    "vt_abi_version": (("test_abi::test_gfx950_library_exports_every_symbol",), None),
    "vt_build_target": (("test_abi::test_gfx950_library_exports_every_symbol",), None),
    "vt_last_error": (("test_ops::test_instnorm_plane_one_launch",), None),
    "vt_upfirdn2d_out_size": (("test_ops::test_upfirdn2d_golden",), ("op.upfirdn2d", "op.upfirdn2d._UpFirDn2d", "op.upfirdn2d._planes",
                                                                  "kernels.upfirdn2d_planes", "kernels.upfirdn2d_out_size")),
    "vt_upfirdn2d": (("test_ops::test_upfirdn2d_golden", f"{NORM}::test_upfirdn2d_gradients"), ("op.upfirdn2d", "op.upfirdn2d._UpFirDn2d", "op.upfirdn2d._planes",
                                                         "kernels.upfirdn2d_planes")),
    "vt_fused_bias_act": (("test_ops::test_fused_leaky_relu_golden_bit_exact", f"{NORM}::test_fused_leaky_relu_gradients",
                           f"{NORM}::test_fused_bias_act_modes_and_forms", f"{NORM}::test_grid_stride_fused_bias_act_flat"), ("op.fused_leaky_relu", "op.fused_act._FusedLeakyReLU",
                                                                                   "kernels.fused_bias_act")),
    "vt_conv2d": (("test_ops::test_conv_fused_torgb",), ("kernels.conv2d",)),
    "vt_conv2d_tile": (("test_ops::test_conv_thin_kernel",), None),
    "vt_conv2d_ws_bytes": (("test_engine::test_style_cache_is_keyed_on_the_callers_tensor",), ("engine.VToonifyEngine",)),
    "vt_conv2d_splitk_mode": (("test_ops::test_conv_splitk_in_launch_equals_two_pass",), None),
    "vt_conv_weight_stream_bytes": (("test_ops::test_conv_whole_k_kernel",), ("kernels.conv_weight_stream",)),
    "vt_conv_tile_stats_bytes": (("test_ops::test_conv_whole_k_adain_chain",), ("kernels.conv_tile_stats_bytes",)),
    "vt_conv_weight_stream": (("test_ops::test_conv_whole_k_kernel",), ("kernels.conv_weight_stream",)),
    "vt_pack_conv_weight": (("test_ops::test_conv_fused_torgb",), ("kernels.pack_conv_weight",)),
    "vt_modulate_weight": ((f"{GLUE}::test_modulate_weight_batch", "test_ops::test_styled_conv_golden"), None),
    "vt_linear": (("test_ops::test_linear_pixelnorm",), ("kernels.linear",)),
    "vt_linear_batch": ((f"{GLUE}::test_linear_batch",), None),
    "vt_modulate_weight_batch": ((f"{GLUE}::test_modulate_weight_batch",), None),
    "vt_pixel_norm": ((f"{GLUE}::test_pixel_norm", "test_ops::test_linear_pixelnorm"), None),
    "vt_style_gate": ((f"{GLUE}::test_style_gate", "test_engine::test_style_gate_is_transparent"), None),
    "vt_linear_batch_gated": ((f"{GLUE}::test_linear_batch",), None),
    "vt_modulate_weight_batch_gated": ((f"{GLUE}::test_modulate_weight_batch",), None),
    "vt_pixel_norm_gated": ((f"{GLUE}::test_pixel_norm",), None),
    "vt_instnorm_ws_bytes": ((f"{GLUE}::test_channel_mean",), ("kernels.instnorm_ws_bytes",)),
    "vt_instnorm_stats": (("test_ops::test_instnorm_adain_fusion_pack", f"{NORM}::test_instnorm_chunked_shapes",
                           f"{NORM}::test_instnorm_chunked_numerics", f"{NORM}::test_instnorm_constant_plane"), ("kernels.instnorm_stats",)),
    "vt_instnorm_apply": (("test_ops::test_conv_emits_instnorm_records", f"{NORM}::test_instnorm_chunked_shapes",
                           f"{NORM}::test_instnorm_chunked_numerics", f"{NORM}::test_instnorm_apply_plane_limit"), None),
    "vt_instnorm_apply_stats": (("test_ops::test_conv_emits_instnorm_records", f"{NORM}::test_instnorm_chunked_shapes",
                                 f"{NORM}::test_instnorm_apply_plane_limit"), None),
    "vt_instnorm_plane": (("test_ops::test_instnorm_plane_one_launch", f"{NORM}::test_instnorm_plane",
                           f"{NORM}::test_instnorm_constant_plane"), None),
    "vt_affine_apply": (("test_ops::test_instnorm_adain_fusion_pack", f"{NORM}::test_instnorm_chunked_shapes",
                         f"{NORM}::test_grid_stride_affine_apply_fusion_pack"), ("kernels.affine_apply",)),
    "vt_fusion_pack": (("test_ops::test_instnorm_adain_fusion_pack", f"{NORM}::test_fusion_pack",
                        f"{NORM}::test_grid_stride_affine_apply_fusion_pack"), ("kernels.fusion_pack",)),
    "vt_frame_pack": (("test_video::test_frame_pack_unpack_vs_oracle", f"{NORM}::test_frame_pack", f"{NORM}::test_grid_stride_frame_io"), ("video.frame_pack",)),
    "vt_frame_unpack": (("test_video::test_frame_pack_unpack_vs_oracle", f"{NORM}::test_frame_unpack",
                         f"{NORM}::test_grid_stride_frame_io"), ("video.frame_unpack",)),
    "vt_channel_mean": ((f"{GLUE}::test_channel_mean",), None),
    "vt_se_apply": ((f"{GLUE}::test_se_apply",), None),
    "vt_upsample_bilinear_add": ((f"{GLUE}::test_upsample_bilinear_add", f"{GLUE}::test_grid_stride_upsample_bilinear_add"),
                                 None),
    "vt_maxpool2d": ((f"{GLUE}::test_maxpool2d",), None),
    "vt_gate_add_nearest": ((f"{GLUE}::test_gate_add_nearest",), None),
    "vt_resize_bilinear": ((f"{GLUE}::test_resize_bilinear",), None),
    "vt_corr_lookup": ((f"{GLUE}::test_corr_lookup",), None),
    "vt_avgpool2x2": ((f"{GLUE}::test_avgpool2x2", f"{GLUE}::test_grid_stride_avgpool2x2"), None),
    "vt_flow_warp": ((f"{GLUE}::test_flow_warp",), None),
    "vt_parsing_fuse": ((f"{GLUE}::test_parsing_fuse",), None),
    "vt_eltwise2": ((f"{GLUE}::test_grid_stride_eltwise2_gru_blend", "test_raft_net::test_glue_kernels"), None),
    "vt_gru_blend": ((f"{GLUE}::test_grid_stride_eltwise2_gru_blend", "test_raft_net::test_glue_kernels"), None),
    "vt_coords_from_flow": (("test_raft_net::test_glue_kernels", f"{NORM}::test_raft_glue_kernels", f"{NORM}::test_grid_stride_raft_glue"),
                            None),
    "vt_convex_upsample": (("test_raft_net::test_glue_kernels", f"{NORM}::test_raft_glue_kernels", f"{NORM}::test_grid_stride_raft_glue"),
                           None),
    "vt_nchw_to_nhwc": (("test_ops::test_layout_change_at_the_model_boundary",), ("kernels.nchw_to_nhwc",)),
    "vt_nhwc_to_nchw": (("test_ops::test_layout_change_back_to_planes",), None),
    "vt_mfma_selftest": (("test_ops::test_mfma_lane_maps",), ("kernels.mfma_selftest",)),
}


def _test_source(test_id):
    """Source of the test function and of the module-level helpers it calls."""
    mod, fn = test_id.split("::")
    path = os.path.join(REPO, "tests", mod + ".py")
    assert os.path.exists(path), f"{test_id}: no tests/{mod}.py"
    src = open(path).read()
    defs = {node.name: node for node in ast.parse(src).body if isinstance(node, ast.FunctionDef)}
    assert fn in defs, f"{test_id}: no such test function"
    called = {c.func.id for c in ast.walk(defs[fn]) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
    return "\n".join(ast.get_source_segment(src, defs[f]) for f in [fn] + sorted(called & set(defs) - {fn}))


def test_every_entry_point_has_a_test():
    from test_abi import _declared
    assert sorted(COVERED) == _declared(), "COVERED must list exactly the entry points of include/vtoonify_amd.h"
    for name, (tests, chain) in COVERED.items():
        assert tests, name
        for t in tests:
            assert t.split("::")[1].startswith("test_"), t
        srcs = [_test_source(t) for t in tests]
        if chain is None:
            assert any(re.search(rf"\b{name}\b", s) for s in srcs), f"{name}: none of {tests} mentions it"
            continue
        first = chain[0].rsplit(".", 1)[1]
        assert any(re.search(rf"\b{first}\(", s) for s in srcs), f"{name}: none of {tests} calls {chain[0]}"
        for i, w in enumerate(chain):
            mod, fn = w.rsplit(".", 1)
            wsrc = inspect.getsource(getattr(importlib.import_module("vtoonify_amd." + mod), fn))
            target = name if i == len(chain) - 1 else chain[i + 1].rsplit(".", 1)[1]
            assert re.search(rf"\b{target}\b", wsrc), f"{name}: vtoonify_amd.{w} does not reach {target}"
