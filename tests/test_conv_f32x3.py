"""vt_conv_desc.dtype = VT_F32X3, kernel family by kernel family, per element against a float64 model of the split.

f32x3 (conv_igemm.hip, "f32x3") splits every fp32 operand x in the fragment registers into h = rne_bf16(x) and
l = rne_bf16(fp32(x - h)) and issues a*b as ah*bh + al*bh + ah*bl on the bf16 matrix cores with fp32 accumulation.  The split
is deterministic arithmetic, so the reference here is not an fp32 oracle but the split itself, evaluated in float64:

    model = conv(xh, wh) + conv(xl, wh) + conv(xh, wl)        what the kernel is meant to compute (al*bl is dropped)
    exact = conv(x, w)
    S     = conv(|x|, |w|)                                     the magnitudes behind each output element

followed by the descriptor's epilogue (bias, LeakyReLU, gain * alpha, residual; the 4x4 FIR of the up-sampling form; the
AdaIN affine of the whole-K loader) in float64, the gain folded into S.  Two per-element bounds:

  * model against exact, CPU only:  |model - exact| <= 2^-16 S.  Per product the worst case is larger -- |x - h - l| can
    reach 2^-17 |x| for either operand and the dropped al*bl 2^-16 |a*b|, 2^-15 in all -- but that needs every remainder of
    a sum at its rounding boundary with one sign; over the >= 64 x k x k products of an output element here the residuals
    are those of independent roundings and come to 0.03 .. 0.10 of 2^-16 S, so 2^-16 S holds with a factor of ten to spare
    and still fails a model that loses a whole term (2^-9 S).
  * kernel against model: only the fp32 accumulation order remains.  Its constant is not chosen here: the same three-term
    model is evaluated with torch float32 convs (and the float32 epilogue), tau = max_i |model32_i - model_i| / S_i is that
    evaluation's own error, and the kernel passes if |y_i - model_i| <= 4 tau S_i + 1e-30 for EVERY element.  The factor 4
    is for a summation tree that is not torch's: 32-channel rows, nine taps, eight waves summed through LDS, split-K slabs.

test_wrong_models_violate_the_bound shows on the same inputs that this bar bites: a model without the xl*wh term, and one
whose remainders are taken from the neighbouring element of each pair, are both far outside it.

With integer operands of 9 to 11 significant bits (h + l == x exactly, l != 0) and S < 2^24 every partial sum is an integer
below 2^24, the order does not matter, and kernel == model BIT FOR BIT, the dropped al*bl included; x * 2^12 and w * 2^-7
must give bitwise 2^5 times the output (no reference at all: any absolute threshold or mishandled exponent in the split).

Every case pins its plan (vt_conv2d_tile), that the f32x3 instance ran (bits differ from the VT_F32 run) or that the
descriptor fell back (bits equal to the VT_F32 run / VT_ERR_UNSUPPORTED with nothing written), and surrounds its output with
NaN sentinels: slack channels per pixel (ld_out = cout rounded up to 8, plus 8) and a tail behind the buffer.

Measured (profiles/f32x3_kernels.txt): tau 0.3 .. 1.1 x 2^-24, kernels 0.4 .. 1.7 x 2^-24 S on the MI355X (at most 2.3 tau) and
0.5 .. 2.0 on the emulation (at most 3.9 tau: its MFMA is one fp32 addition per product).  The 1-D and patch kernels were at
2.0 .. 3.0 (MI355X; 4.2 and 4.8 tau on two cases) and 4.6 .. 7.3 (emulation) while their three MFMAs per row were chained on the
accumulator of the whole K range; Mma<f32x3_t>::run3_row sums a row from zero and adds it once.

With VT_F32X3_REPORT=<file> every case appends one line (plan code, ran / fallback, tau and the kernel's worst |y - model| / S
in units of 2^-24) -- profiles/f32x3_kernels.txt is that file from a host-emulation run and from an MI355X run.
"""
import ctypes as C
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtoonify_amd import _lib, kernels as K

P = 100000000                 # tile-code digit of the kernel family (vt_conv2d_tile)
U24 = 2.0 ** -24
L = K.ACT_LRELU
UNSUPPORTED = 2               # VT_ERR_UNSUPPORTED
TAIL = 64                     # NaN elements behind every output buffer
K1 = np.array([1, 3, 3, 1], np.float32)
FIR_STD = (np.outer(K1, K1) / 64.0 * 4.0).astype(np.float32)                                    # make_kernel([1,3,3,1]) * up^2
FIR_ODD = (np.outer(K1, np.array([0.9, 3.1, 2.7, 1.3], np.float32)) / 64.0 * 4.0).astype(np.float32)   # taps that are no bf16 numbers


# ------------------------------------------------------------------------------------------------ the split, in numpy
def rne_bf16(a):
    """fp32 array -> the nearest bf16 values (ties to even), held in fp32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def x3_split(a):
    """x3_split of conv_igemm.hip: h = rne_bf16(x), l = rne_bf16(fp32(x - h))."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    h = rne_bf16(a)
    return h, rne_bf16((a - h).astype(np.float32))


def test_split_helper():
    g = np.random.default_rng(1)
    a = (g.standard_normal(4096) * 10.0 ** g.integers(-6, 6, 4096)).astype(np.float32)
    h, l = x3_split(a)
    assert np.array_equal(h, torch.from_numpy(a).to(torch.bfloat16).float().numpy())           # the same RNE as torch's
    assert np.array_equal(l, torch.from_numpy(a - h).to(torch.bfloat16).float().numpy())
    assert np.all(np.abs(a.astype(np.float64) - h - l) <= 2.0 ** -17 * np.abs(a))               # conv_igemm.hip, "f32x3"
    t = np.array([257.0, 259.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)              # ties: to the even neighbour
    assert np.array_equal(rne_bf16(t), np.array([256.0, 260.0, 1.0, 1.0 + 2.0 ** -6], np.float32))


# ------------------------------------------------------------------------------------------------------------ cases
def case(name, N, c0, H, W, cout, **kw):
    d = dict(name=name, N=N, c0=c0, c1=0, H=H, W=W, cout=cout, k=3, stride=1, dil=1, pad=None, act=0, gain=1.0, resid=False,
             alpha=1.0, beta=0.0, alpha_dev=None, planar=False, hint=0, ws=False, stream=False, two_pass=False, transposed=False,
             fir=None, env={}, bias=True, kind=None, tile=None, splitk=None, x3=True, seed=0, zero_ch=0)
    assert not set(kw) - set(d), set(kw) - set(d)
    d.update(kw)
    c = SimpleNamespace(**d)
    if c.pad is None:
        c.pad = c.dil * (c.k // 2)
    if c.act == L:
        c.gain = 2 ** 0.5
    if c.resid:
        c.alpha, c.beta = 0.5, 0.25
    c.cin = c.c0 + c.c1
    if c.fir is not None:
        c.Ho, c.Wo = 2 * H, 2 * W
    elif c.transposed:
        c.Ho, c.Wo = 2 * H + 1, 2 * W + 1
    else:
        c.Ho = (H + 2 * c.pad - c.dil * (c.k - 1) - 1) // c.stride + 1
        c.Wo = (W + 2 * c.pad - c.dil * (c.k - 1) - 1) // c.stride + 1
    c.seed = c.seed or (sum(map(ord, name)) % 1000 + 1)
    return c


ONE_D = [case(f"1d {t // 1000}x{t % 1000}", 2, 64, 13, 10, 136, act=L, resid=True, hint=2 * P + t, kind=2, tile=t, splitk=1)
         for t in (128128, 128064, 128032, 128016, 64064, 64128, 32064)] + [
    case("1d 64x64 split-K 4 + reduce", 2, 64, 13, 10, 136, act=L, resid=True, hint=2 * P + 4000000 + 64064, ws=True,
         kind=2, tile=64064, splitk=4),
    case("1d 64x64 split-K 4, two passes", 2, 64, 13, 10, 136, act=L, resid=True, hint=2 * P + 4000000 + 64064, ws=True,
         two_pass=True, kind=2, tile=64064, splitk=4),
    case("1d stride 2", 1, 64, 13, 18, 72, stride=2, act=L, ws=True, kind=2),
    case("1d 1x1", 2, 64, 9, 7, 8, k=1, ws=True, kind=2),
]
PATCH = [case(f"patch {t // 1000}x{t % 1000}", 1, 128, 21, 35, 136, resid=True, act=L, hint=P + t, kind=1, tile=t, splitk=1)
         for t in (256128, 256064, 128064, 128016)] + [
    case("patch 128x128 auto split", 1, 128, 21, 35, 136, resid=True, act=L, hint=P + 128128, ws=True, kind=1, tile=128128),
    case("patch 128x128 ABUF 2 (4 chunks per slice)", 1, 128, 21, 35, 136, resid=True, act=L, hint=P + 1000000 + 128128, ws=True,
         kind=1, tile=128128, splitk=1),
    case("patch 128x128 ABUF 1 (1 chunk per slice)", 1, 128, 21, 35, 136, resid=True, act=L, hint=P + 4000000 + 128128, ws=True,
         kind=1, tile=128128, splitk=4),
    case("patch two sources 96 + 32", 1, 96, 21, 35, 136, c1=32, resid=True, act=L, hint=P + 128064, kind=1, tile=128064),
    case("patch planar fp32 output", 1, 128, 21, 35, 8, planar=True, hint=P + 128016, kind=1, tile=128016),
    case("patch 128x128 dil 2 (no f32x3 instance)", 1, 128, 21, 35, 136, dil=2, resid=True, act=L, hint=P + 128128, ws=True,
         kind=1, tile=128128, x3=False),
    case("patch 128x128 dil 4 (no f32x3 instance)", 1, 128, 21, 35, 136, dil=4, resid=True, act=L, hint=P + 128128, ws=True,
         kind=1, tile=128128, x3=False),
    case("patch transposed by parity (no f32x3 instance)", 2, 128, 9, 21, 72, transposed=True, stride=2, pad=0, bias=False,
         kind=1, tile=256064, x3=False),
]
WHOLE_K = [
    case("whole-K one round, residual, alpha_dev", 2, 256, 9, 11, 136, stream=True, act=L, resid=True, alpha_dev=0.625,
         hint=4 * P, kind=4),
    case("whole-K two rounds", 1, 512, 9, 11, 40, stream=True, act=L, hint=4 * P, kind=4),
    case("whole-K three rounds", 1, 768, 8, 8, 40, stream=True, hint=4 * P, kind=4),
    case("whole-K dil 2", 1, 256, 12, 10, 40, stream=True, dil=2, act=L, hint=4 * P, kind=4),
    case("whole-K dil 4", 1, 256, 12, 10, 40, stream=True, dil=4, resid=True, hint=4 * P, kind=4),
    case("whole-K two sources 128 + 128", 1, 128, 9, 11, 40, c1=128, stream=True, hint=4 * P, kind=4),
    case("whole-K planar fp32 output", 1, 256, 9, 11, 8, stream=True, planar=True, hint=4 * P, kind=4),
]
UPBLUR = [c for fn, fir in (("1331", FIR_STD), ("odd", FIR_ODD)) for c in (
    case(f"upblur 32-channel tiles, single stage, LB2 / {fn}", 2, 64, 11, 16, 40, fir=fir, act=L, hint=32, kind=5, tile=32),
    case(f"upblur 16-channel tiles, single stage / {fn}", 1, 32, 13, 3, 32, fir=fir, act=L, hint=0, kind=5, tile=16),
    case(f"upblur 16-channel tiles, double-buffered / {fn}", 1, 160, 6, 9, 32, fir=fir, act=L, hint=16, kind=5, tile=16),
    case(f"upblur 32-channel tiles, double-buffered / {fn}", 1, 128, 27, 15, 32, fir=fir, act=L, hint=32, kind=5, tile=32,
         env={"VT_UPBLUR_DB": "4"}))]
NO_X3 = [   # kernels without an f32x3 instance: the launch must be the VT_F32 one
    case("thin outputs 3x3 (no f32x3 instance)", 1, 64, 9, 9, 3, planar=True, kind=6, x3=False),
    case("thin outputs 1x1 (no f32x3 instance)", 2, 64, 7, 5, 3, k=1, planar=True, kind=6, x3=False),
    case("register-staged stem, 22 -> 24 channels (no f32x3 instance)", 1, 24, 12, 9, 32, act=L, zero_ch=2, kind=0, x3=False),
]
GAUSS = ONE_D + PATCH + WHOLE_K + UPBLUR + NO_X3


# -------------------------------------------------------------------------------------------- the float64 / float32 models
def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def lin(c, x, w):
    """The linear part of case c on torch tensors x (N, cin, H, W), w (cout, cin, k, k) of one float dtype."""
    if c.fir is not None:
        z = F.conv_transpose2d(x, w.permute(1, 0, 2, 3), stride=2)                       # (2H+1, 2W+1)
        n, co, zh, zw = z.shape
        fir = torch.from_numpy(c.fir).to(x.dtype).flip(0, 1)[None, None]                 # upfirdn2d: the flipped kernel, pad (1, 1)
        return F.conv2d(F.pad(z, (1, 1, 1, 1)).reshape(n * co, 1, zh + 2, zw + 2), fir).reshape(n, co, zh - 1, zw - 1)
    if c.transposed:
        return F.conv_transpose2d(x, w.permute(1, 0, 2, 3), stride=2)
    return F.conv2d(x, w, None, c.stride, c.pad, c.dil)


def ga_of(c):
    """gain * alpha * alpha_dev as the library forms it: fp32 products."""
    ga = np.float32(np.float32(c.gain) * np.float32(c.alpha))
    return float(ga * np.float32(c.alpha_dev) if c.alpha_dev is not None else ga)


def epilogue(c, v, b, r, dt):
    """act(v + bias) * gain * alpha * alpha_dev + beta * resid in dtype dt (descriptor values as the fp32 the library sees)."""
    if b is not None:
        v = v + _t(b, dt).view(1, -1, 1, 1)
    if c.act == L:
        v = torch.where(v > 0, v, v * float(np.float32(0.2)))
    v = v * ga_of(c)
    if r is not None:
        v = v + float(np.float32(c.beta)) * _t(r, dt)
    return v


def three_terms(c, x, w, dt, xl=None, drop_xl=False):
    """conv(xh, wh) + conv(xl, wh) + conv(xh, wl) in dtype dt.  xl / drop_xl: the deliberately wrong variants."""
    xh, xl0 = x3_split(x)
    wh, wl = x3_split(w)
    xl = xl0 if xl is None else xl
    v = lin(c, _t(xh, dt), _t(wh, dt))
    if not drop_xl:
        v = v + lin(c, _t(xl, dt), _t(wh, dt))
    return v + lin(c, _t(xh, dt), _t(wl, dt))


def reference(c, x, w, b, r):
    """-> model, exact, S (float64 tensors, the epilogue applied, its gain folded into S) and tau."""
    f64, f32 = torch.float64, torch.float32
    model = epilogue(c, three_terms(c, x, w, f64), b, r, f64)
    exact = epilogue(c, lin(c, _t(x, f64), _t(w, f64)), b, r, f64)
    S = lin(c, _t(np.abs(x), f64), _t(np.abs(w), f64)) * abs(ga_of(c))
    model32 = epilogue(c, three_terms(c, x, w, f32), b, r, f32)
    assert float(S.min()) > 0
    tau = float(((model32.double() - model).abs() / S).max())
    return model, exact, S, tau


def operands(c):
    g = np.random.default_rng(c.seed)
    x = g.standard_normal((c.N, c.cin, c.H, c.W)).astype(np.float32)
    if c.zero_ch:
        x[:, -c.zero_ch:] = 0.0          # channel padding of a tensor whose channel count is no multiple of 8
    w = (g.standard_normal((c.cout, c.cin, c.k, c.k)) / math.sqrt(c.cin * c.k * c.k)).astype(np.float32)
    b = g.standard_normal(c.cout).astype(np.float32) if c.bias else None
    r = g.standard_normal((c.N, c.cout, c.Ho, c.Wo)).astype(np.float32) if c.resid else None
    return x, w, b, r


@functools.lru_cache(maxsize=None)
def gauss_problem(name):
    c = next(c for c in GAUSS if c.name == name)
    x, w, b, r = operands(c)
    return (x, w, b, r) + reference(c, x, w, b, r)


# ------------------------------------------------------------------------------------------------------- the launch
def report(c, dev, code, what, tau=None, ratio=None, note=""):
    path = os.environ.get("VT_F32X3_REPORT")
    if path:
        f = lambda v: "      -" if v is None else f"{v / U24:7.2f}"
        with open(path, "a") as fh:
            fh.write(f"{'gpu' if dev.type == 'cuda' else 'emu'} | {c.name:<58} | {code:>10} | {what:<16} | {f(tau)} | {f(ratio)} | {note}\n")


def launch(c, dev, x, w, b, r, dt_code, store=torch.float32):
    """One vt_conv2d of case c on the fp32 (or `store`) tensors of x, w -> (y (N, cout, Ho, Wo) float64 on the CPU, plan code).
    The output lies in a NaN-filled buffer: 8+ slack channels per pixel and TAIL elements behind the last one."""
    lib = _lib.lib()
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt = K.nchw_to_nhwc(dv(x), store)
    wp = K.pack_conv_weight(dv(w), out_dtype=store)                                       # [cout][tap][cin], values unchanged
    if c.c1:   # the second source in its own tensor with a wider pixel stride; NaN between the pixels
        x1 = torch.full((c.N, c.H, c.W, c.c1 + 16), float("nan"), dtype=store, device=dev)
        x1[..., :c.c1] = xt[..., c.c0:]
        srcs = dict(src0=xt[..., :c.c0].contiguous(), c0=c.c0, ld0=c.c0, src1=x1, c1=c.c1, ld1=c.c1 + 16)
    else:
        srcs = dict(src0=xt, c0=c.c0, ld0=c.c0)
    npix = c.N * c.Ho * c.Wo
    if c.planar:
        ldo = 0
        buf = torch.full((npix * c.cout + TAIL,), float("nan"), dtype=torch.float32, device=dev)
        okw = dict(out=buf, ld_out=0, out_layout=K.OUT_NCHW, out_dtype=K.VT_F32)
    else:
        ldo = (c.cout + 7) // 8 * 8 + 8
        # (fp32 rows, also from 16-bit operands -- but the up-sampling kernels store the compute dtype only)
        ost = store if c.fir is not None else torch.float32
        buf = torch.full((npix * ldo + TAIL,), float("nan"), dtype=ost, device=dev)
        okw = dict(out=buf, ld_out=ldo, out_dtype=K.dt_code(ost))
        if r is not None:
            okw.update(resid=K.nchw_to_nhwc(dv(r), torch.float32, ld_out=ldo), ld_res=ldo)
    keep = [dv(np.array([c.alpha_dev], np.float32))] if c.alpha_dev is not None else []
    kw = dict(n=c.N, h=c.H, w=c.W, out_h=c.Ho, out_w=c.Wo, weight=wp, cout=c.cout, kh=c.k, kw=c.k, stride=c.stride, pad=c.pad,
              dil=c.dil, transposed=int(c.transposed), bias=dv(b) if b is not None else None, act=c.act, gain=c.gain,
              alpha=c.alpha, beta=c.beta, alpha_dev=keep[0] if keep else None, dtype=dt_code, tile_hint=c.hint,
              up_fir=dv(c.fir) if c.fir is not None else None, **srcs, **okw)
    if c.stream:
        kw["weight_stream"] = K.conv_weight_stream(wp)
        assert kw["weight_stream"] is not None
    if c.ws:
        kw["splitk_ws"] = torch.zeros(8 << 20, dtype=torch.float32, device=dev)
    d = K.make_conv_desc(**kw)
    code = lib.vt_conv2d_tile(C.byref(d))
    for phase in ((1, 2) if c.two_pass else (0,)):   # two_pass: the K slices, then the reduce pass, as launches of the caller
        d.splitk_phase = phase
        _lib.check(lib.vt_conv2d(C.byref(d), K._stream(buf)), "vt_conv2d")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    if c.ws:
        assert int(kw["splitk_ws"].view(torch.int32)[:4096].abs().max()) == 0, "split-K tickets not left zero"
    assert bool(torch.isnan(buf[-TAIL:]).all()), "tail behind the buffer written"
    if c.planar:
        y = buf[:-TAIL].view(c.N, c.cout, c.Ho, c.Wo)
    else:
        rows = buf[:-TAIL].view(c.N, c.Ho, c.Wo, ldo)
        assert bool(torch.isnan(rows[..., c.cout:]).all()), "slack channels written"
        y = rows[..., :c.cout].permute(0, 3, 1, 2)
    y = y.float().cpu().contiguous()
    assert bool(torch.isfinite(y).all())
    return y, code


def with_env(c, monkeypatch):
    monkeypatch.setenv("VT_UPBLUR_FLAT", "0")
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)


def check_plan(c, code):
    assert code // P == c.kind, (c.name, code)
    if c.tile is not None:
        assert code % (1000000 if c.tile >= 1000 else 1000) == c.tile, (c.name, code)
    if c.splitk is not None:
        assert (code // 1000000) % 100 == c.splitk, (c.name, code)
    elif c.ws and "auto split" in c.name:
        assert (code // 1000000) % 100 > 1, (c.name, code)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------ 1. Gaussian operands: model, bounds, instances
@pytest.mark.parametrize("name", [c.name for c in GAUSS])
def test_model_against_exact(name):
    """CPU only, no kernel: the three-term model is within 2^-16 S of the exact product, element by element."""
    x, w, b, r, model, exact, S, tau = gauss_problem(name)
    ratio = float(((model - exact).abs() / S).max())
    assert ratio <= 2.0 ** -16, (name, ratio * 2 ** 16)
    assert ratio > 2.0 ** -24 and tau > 0          # ... and is not the exact product: the model really carries the split


@pytest.mark.parametrize("name", [c.name for c in GAUSS])
def test_kernel_against_model(dev, monkeypatch, name):
    c = next(c for c in GAUSS if c.name == name)
    with_env(c, monkeypatch)
    x, w, b, r, model, exact, S, tau = gauss_problem(name)
    y3, code = launch(c, dev, x, w, b, r, K.VT_F32X3)
    y1, code1 = launch(c, dev, x, w, b, r, K.VT_F32)
    assert code == code1
    check_plan(c, code)
    ran = not same_bits(y3, y1)
    r1 = float(((y1.double() - exact).abs() / S).max())
    if c.x3:
        err = (y3.double() - model).abs()
        ratio = float((err / S).max())
        print(f"{name}: plan {code}, tau {tau / U24:.2f}, kernel {ratio / U24:.2f}, exact-fp32 instance {r1 / U24:.2f} (x 2^-24 S)")
        report(c, dev, code, "ran" if ran else "DID NOT RUN", tau, ratio)
        assert ran, "the f32x3 instance did not run: bits of the VT_F32 launch"
        bad = err > 4 * tau * S + 1e-30
        assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements outside 4 tau S: worst {ratio / tau:.2f} tau"
    else:
        report(c, dev, code, "exact fp32 bits" if not ran else "OTHER BITS", None, r1)
        assert not ran, "no f32x3 instance of this plan: the launch must be the VT_F32 one"
        # what ran is the exact-fp32 instance: the same yardstick, against `exact` (its operands are not split)
        assert r1 <= 4 * tau + 1e-30, (name, r1 / U24)


@pytest.mark.parametrize("name", [c.name for c in UPBLUR])
def test_upblur_tile_widths_agree(dev, monkeypatch, name):
    """The 16- and 32-channel tiles of conv_upblur_kernel<f32x3_t> give the same bits (the width follows the batch size)."""
    c = next(c for c in GAUSS if c.name == name)
    with_env(c, monkeypatch)
    x, w, b, r = gauss_problem(name)[:4]
    ya, code_a = launch(c, dev, x, w, b, r, K.VT_F32X3)
    c2 = SimpleNamespace(**{**vars(c), "hint": 32 if code_a % 1000 == 16 else 16})
    yb, code_b = launch(c2, dev, x, w, b, r, K.VT_F32X3)
    assert code_a // P == 5 and code_b // P == 5 and {code_a % 1000, code_b % 1000} == {16, 32}
    assert same_bits(ya, yb)


FAMILY = {"1d": ONE_D[0], "patch": PATCH[2], "whole-K": WHOLE_K[1], "upblur": UPBLUR[1]}


@pytest.mark.parametrize("family", list(FAMILY))
def test_wrong_models_violate_the_bound(family):
    """The bar bites (CPU only): on the inputs of a case, a model without the xl * wh term and a model whose remainders come
    from the neighbouring element of each pair (channels 2i <-> 2i + 1, the two halves of a packed bf16 register) both miss
    |wrong - model| <= 4 tau S -- a kernel that computed either would fail test_kernel_against_model."""
    c = FAMILY[family]
    x, w, b, r, model, exact, S, tau = gauss_problem(c.name)
    f64 = torch.float64
    no_xl = epilogue(c, three_terms(c, x, w, f64, drop_xl=True), b, r, f64)
    xl = x3_split(x)[1]
    swapped = xl.reshape(c.N, c.cin // 2, 2, c.H, c.W)[:, :, ::-1].reshape(x.shape)
    nb = epilogue(c, three_terms(c, x, w, f64, xl=swapped), b, r, f64)
    for what, wrong in (("no xl*wh", no_xl), ("neighbour's remainder", nb)):
        bad = (wrong - model).abs() > 4 * tau * S + 1e-30
        assert float(bad.double().mean()) > 0.9, (family, what, float(bad.double().mean()))


# ----------------------------------------------------------------------------------- 2. integer operands: bit for bit
def int_case(family):
    c0 = FAMILY[family]
    return SimpleNamespace(**{**vars(c0), "act": 0, "gain": 1.0, "resid": False, "alpha": 1.0, "beta": 0.0, "bias": False,
                              "fir": FIR_STD if c0.fir is not None else None})


def int_operands(c, bits_lo, bits_hi, per_class):
    """Dense integer activations and sparse integer weights, every non-zero value odd with bits_lo..bits_hi significant bits.
    Weights: per output channel `per_class` non-zero taps in every parity class of the 3x3 window (so a transposed conv sums
    `per_class` products per output element, a plain conv 4 * per_class)."""
    g = np.random.default_rng(c.seed + 17)

    def val(shape):
        m = g.integers(2 ** (bits_lo - 1), 2 ** bits_hi, shape) | 1
        return (m * g.choice([-1, 1], shape)).astype(np.float32)
    x = val((c.N, c.cin, c.H, c.W))
    w = np.zeros((c.cout, c.cin, 3, 3), np.float32)
    classes = [[(0, 0), (0, 2), (2, 0), (2, 2)], [(0, 1), (2, 1)], [(1, 0), (1, 2)], [(1, 1)]]
    for co in range(c.cout):
        for cls in classes:
            for _ in range(per_class):
                a, bb = cls[g.integers(len(cls))]
                w[co, g.integers(c.cin), a, bb] = val(())
    return x, w


def int_problem(c, bits_lo, bits_hi):
    x, w = int_operands(c, bits_lo, bits_hi, 1)
    f64 = torch.float64
    model = three_terms(c, x, w, f64)
    S = lin(c, _t(np.abs(x), f64), _t(np.abs(w), f64))
    quantum = 1.0 / 16 if c.fir is not None else 1.0         # FIR_STD: taps k / 16, separable as (k / 8) x (k / 2)
    return x, w, model, S, quantum


@pytest.mark.parametrize("family", list(FAMILY))
def test_integer_operands_are_well_posed(family):
    """CPU only: the operands of the integer cases split exactly with l != 0, and every partial sum is an integer (a
    multiple of 1/16 behind the FIR) below 2^24 of its unit -- so fp32 accumulation in any order is exact."""
    c = int_case(family)
    for lo, hi in ((9, 9),) if c.fir is not None else ((9, 11),):
        x, w, model, S, quantum = int_problem(c, lo, hi)
        assert float(S.max()) / quantum < 2 ** 24, (family, float(S.max()))
        for a in (x, w):
            h, l = x3_split(a)
            nz = a != 0
            assert np.array_equal(h.astype(np.float64) + l, a.astype(np.float64))
            assert (l[nz] != 0).mean() >= 0.25
        assert (w != 0).sum() >= 3 * c.cout
        assert bool((model == model.float().double()).all())             # the model itself is an fp32 number
        exact = lin(c, _t(x, torch.float64), _t(w, torch.float64))
        assert bool((model != exact).any())                               # the dropped xl * wl shows


@pytest.mark.parametrize("family", list(FAMILY))
def test_integer_operands_bit_exact(dev, monkeypatch, family):
    """No bias, no activation, gain 1: kernel == model bit for bit, the dropped al * bl included.  Control for the premise
    (the MFMA adds exactly representable integers below 2^24 without loss): the same conv on the plain bf16 instance with
    operands of at most 8 bits and denser weights."""
    c = int_case(family)
    with_env(c, monkeypatch)
    # control: bf16 tensors, 8-bit operands, 16 taps per parity class (sums of ~1e6, < 2^24), the same plan family
    cb = SimpleNamespace(**{**vars(c), "c0": max(c.c0, 64), "cin": max(c.cin, 64)})     # (the K unit of bf16 is 64 channels)
    # (the 16-bit up-sampling kernels keep their z tile in the compute dtype and store bf16 rows: operands of at most 4 bits
    # and one product per z element, so that z is a bf16 number and the stored row the one rounding of the exact value)
    xb, wb = int_operands(cb, 1, 4 if c.fir is not None else 8, 1 if c.fir is not None else 16)
    Sb = lin(cb, _t(np.abs(xb), torch.float64), _t(np.abs(wb), torch.float64))
    quantum = 1.0 / 16 if c.fir is not None else 1.0
    assert float(Sb.max()) / quantum < 2 ** 24
    want_b = lin(cb, _t(xb, torch.float64), _t(wb, torch.float64))
    yb, code_b = launch(cb, dev, xb, wb, None, None, K.VT_BF16, store=torch.bfloat16)
    assert code_b // P == c.kind, code_b
    if c.fir is not None:
        want_b = want_b.float().to(torch.bfloat16).double()
    control = bool((yb.double() == want_b).all())
    report(c, dev, code_b, "control exact" if control else "CONTROL INEXACT", note="integer control, bf16 instance, operands <= 8 bits")
    assert control, "integer sums below 2^24 on the bf16 MFMA are not exact"
    lo, hi = (9, 9) if c.fir is not None else (9, 11)
    x, w, model, S, quantum = int_problem(c, lo, hi)
    y, code = launch(c, dev, x, w, None, None, K.VT_F32X3)
    check_plan(c, code)
    diff = int((y.double() != model).sum())
    report(c, dev, code, "bit-exact" if diff == 0 else "NOT EXACT", note=f"integer operands, {lo}..{hi} significant bits")
    assert diff == 0, f"{diff} of {y.numel()} elements differ from the model"


@pytest.mark.parametrize("family", list(FAMILY))
def test_scale_equivariance(dev, monkeypatch, family):
    """x * 2^12 and w * 2^-7, no bias: bitwise 2^5 times the unscaled output (LeakyReLU and the gain are homogeneous)."""
    c0 = FAMILY[family]
    c = SimpleNamespace(**{**vars(c0), "bias": False, "resid": False, "alpha": 1.0, "beta": 0.0})
    with_env(c, monkeypatch)
    x, w = gauss_problem(c0.name)[:2]
    y, code = launch(c, dev, x, w, None, None, K.VT_F32X3)
    ys, _ = launch(c, dev, x * np.float32(2.0 ** 12), w * np.float32(2.0 ** -7), None, None, K.VT_F32X3)
    check_plan(c, code)
    assert float(y.abs().max()) > 0.1 and same_bits(ys, y * 32.0), family


# ------------------------------------------------------------- 3. whole-K: tile_stats out, the AdaIN prologue in, in f32x3
def bound_check(name, dev, code, y, model, S, tau):
    err = (y.double() - model).abs()
    ratio = float((err / S).max())
    print(f"{name}: plan {code}, tau {tau / U24:.2f}, kernel {ratio / U24:.2f} (x 2^-24 S)")
    report(SimpleNamespace(name=name), dev, code, "ran", tau, ratio)
    bad = err > 4 * tau * S + 1e-30
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} elements outside 4 tau S: worst {ratio / tau:.2f} tau"


@pytest.mark.parametrize("N,H,W,dA,dB", [(2, 17, 11, 1, 2), (2, 9, 20, 4, 1)])
def test_whole_k_adain_chain(dev, N, H, W, dA, dB):
    """The AdaResBlock chain of test_ops.py::test_conv_whole_k_adain_chain with both convs in f32x3: conv A stores its output
    and the per-tile {mean, M2} records (tile_stats); conv B merges them, rewrites its patch in LDS as AdaIN(x) -- in fp32,
    BEFORE the split -- and convolves.  Conv A against its model; the records against float64 statistics of the kernel's
    own output; conv B against the model of conv(AdaIN(stored A)), with scale / shift formed from the records the way the
    loader forms them (merge in float64, rstd, scale and shift rounded to fp32, x * scale + shift as one fma)."""
    lib = _lib.lib()
    Cc, Co = 256, 40
    cA = case(f"whole-K adain chain A, dil {dA}, tile_stats out", N, Cc, H, W, Cc, stream=True, dil=dA, act=L, hint=4 * P, kind=4,
              seed=91 + dA)
    x, wA, bA, _ = operands(cA)
    g = np.random.default_rng(7 + dB)
    wB = (g.standard_normal((Co, Cc, 3, 3)) / math.sqrt(Cc * 9)).astype(np.float32)
    gb = (1.0 + 0.3 * g.standard_normal((N, 2 * Cc))).astype(np.float32)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt = K.nchw_to_nhwc(dv(x), torch.float32)
    wpA, wpB = K.pack_conv_weight(dv(wA)), K.pack_conv_weight(dv(wB))
    nrec = K.conv_tile_stats_bytes(N, H, W, dA, Cc) // 4
    ts = torch.full((nrec + TAIL,), float("nan"), dtype=torch.float32, device=dev)
    ldo = Cc                                    # (tile_stats: the tensor conv B reads -- rows of exactly C channels)
    bufA = torch.full((N * H * W * ldo + TAIL,), float("nan"), dtype=torch.float32, device=dev)
    kwA = dict(src0=xt, c0=Cc, ld0=Cc, n=N, h=H, w=W, out_h=H, out_w=W, weight=wpA, weight_stream=K.conv_weight_stream(wpA),
               cout=Cc, kh=3, kw=3, pad=dA, dil=dA, bias=dv(bA), act=L, gain=cA.gain, out=bufA, ld_out=ldo, tile_stats=ts,
               tile_hint=4 * P)
    outs = {}
    for dt in (K.VT_F32, K.VT_F32X3):          # (f32x3 last: its output and records stay in bufA / ts for conv B)
        bufA.fill_(float("nan"))
        ts.fill_(float("nan"))
        d = K.make_conv_desc(dtype=dt, **kwA)
        codeA = lib.vt_conv2d_tile(C.byref(d))
        assert codeA // P == 4, codeA
        _lib.check(lib.vt_conv2d(C.byref(d), K._stream(bufA)), "conv A")
        assert bool(torch.isnan(bufA[-TAIL:]).all()) and bool(torch.isnan(ts[-TAIL:]).all()), "tail written"
        outs[dt] = bufA[:-TAIL].view(N, H, W, Cc).permute(0, 3, 1, 2).cpu().contiguous()
    a = outs[K.VT_F32X3]
    assert bool(torch.isfinite(a).all()) and not same_bits(a, outs[K.VT_F32]), "conv A: the f32x3 instance did not run"
    modelA, exactA, SA, tauA = reference(cA, x, wA, bA, None)
    bound_check(cA.name, dev, codeA, a, modelA, SA, tauA)

    # ---- the records: tile (phase_y, phase_x, tile_y, tile_x) of dilation dA, {mean, M2} per channel, then the pixel counts
    ty, tx = -(-(-(-H // dA)) // 8), -(-(-(-W // dA)) // 8)
    nt = dA * dA * ty * tx
    tsc = ts[:-TAIL].cpu().numpy()
    rec = tsc[:N * nt * Cc * 2].reshape(N, nt, Cc, 2).astype(np.float64)
    cnt = tsc[N * nt * Cc * 2:].reshape(N, nt).astype(np.float64)
    a64 = a.double().numpy()
    for n in range(N):
        ti = 0
        for fy in range(dA):
            for fx in range(dA):
                for iy in range(ty):
                    for ix in range(tx):
                        blk = a64[n, :, fy + iy * 8 * dA::dA, fx + ix * 8 * dA::dA][:, :8, :8].reshape(Cc, -1)
                        k = blk.shape[1]
                        assert cnt[n, ti] == k
                        if k:
                            # fp32 sums of k <= 64 terms, a division, a store: (k + 2) roundings of 2^-24 relative to sum|.|
                            m = blk.mean(1)
                            assert np.all(np.abs(rec[n, ti, :, 0] - m) <= (k + 2) * U24 * np.abs(blk).mean(1) + 1e-30)
                            m2 = ((blk - m[:, None]) ** 2).sum(1)
                            # ... and of the squares, each (a - mean)^2 with 3 more roundings and the mean's error in it
                            assert np.all(np.abs(rec[n, ti, :, 1] - m2) <= (k + 8) * U24 * (m2 + np.abs(blk).mean(1) ** 2) + 1e-30)
                        ti += 1
    # ---- AdaIN as the loader of conv B forms it (conv_fullk.hpp): merge of the records in float64, shifted by tile 0's mean
    hw = float(H * W)
    x0 = rec[:, 0, :, 0]
    dm = rec[..., 0] - x0[:, None, :]
    s1 = (cnt[:, :, None] * dm).sum(1)
    s2 = (np.where(cnt[:, :, None] > 0, rec[..., 1], 0.0) + cnt[:, :, None] * dm * dm).sum(1)
    mean = x0 + s1 / hw
    var = np.maximum((s2 - s1 * s1 / hw) / hw, 0.0)
    f32 = np.float32
    rstd = (1.0 / np.sqrt(var + float(f32(1e-5)))).astype(f32)
    scale = gb[:, :Cc] * rstd                                                        # fp32 products
    shift = gb[:, Cc:] - scale * mean.astype(f32)
    an = (a64 * scale.astype(np.float64)[:, :, None, None] + shift.astype(np.float64)[:, :, None, None]).astype(f32)
    # (the same statistics from the stored tensor itself, in float64: the records carry them to fp32 accuracy)
    assert np.abs(mean - a64.mean((2, 3))).max() <= 1e-5 and np.abs(var / a64.var((2, 3)) - 1).max() <= 1e-4

    cB = case(f"whole-K adain chain B, dil {dB}, stats of dil {dA} in", N, Cc, H, W, Co, stream=True, dil=dB, bias=False,
              hint=4 * P, kind=4)
    modelB, exactB, SB, tauB = reference(cB, an, wB, None, None)
    ldb = Co + 8
    outsB = {}
    wsB, gbt = K.conv_weight_stream(wpB), dv(gb)
    for dt in (K.VT_F32X3, K.VT_F32):
        bufB = torch.full((N * H * W * ldb + TAIL,), float("nan"), dtype=torch.float32, device=dev)
        d = K.make_conv_desc(src0=bufA, c0=Cc, ld0=Cc, n=N, h=H, w=W, out_h=H, out_w=W, weight=wpB, weight_stream=wsB,
                             cout=Co, kh=3, kw=3, pad=dB, dil=dB, out=bufB, ld_out=ldb, dtype=dt, tile_hint=4 * P,
                             in_tile_stats=ts, in_stats_dil=dA, in_gb=gbt, in_ld_gb=2 * Cc)
        codeB = lib.vt_conv2d_tile(C.byref(d))
        assert codeB // P == 4, codeB
        _lib.check(lib.vt_conv2d(C.byref(d), K._stream(bufB)), "conv B")
        rows = bufB[:-TAIL].view(N, H, W, ldb)
        assert bool(torch.isnan(bufB[-TAIL:]).all()) and bool(torch.isnan(rows[..., Co:]).all()), "slack written"
        outsB[dt] = rows[..., :Co].permute(0, 3, 1, 2).cpu().contiguous()
    assert same_bits(bufA[:-TAIL].view(N, H, W, Cc).permute(0, 3, 1, 2).cpu().contiguous(), a), "conv B wrote its input"
    assert not same_bits(outsB[K.VT_F32X3], outsB[K.VT_F32]), "conv B: the f32x3 instance did not run"
    bound_check(cB.name, dev, codeB, outsB[K.VT_F32X3], modelB, SB, tauB)


# --------------------------------------------------------------------------- 4. descriptors that have no f32x3 form
def nan_buf(n, dev):
    return torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device=dev)


def strided(t, ld, dev):
    """(n, h, w, c) values in NaN-filled pixel rows of ld elements, + tail."""
    n, h, w, c = t.shape
    buf = torch.full((n * h * w * ld + TAIL,), float("nan"), dtype=torch.float32)
    buf[:n * h * w * ld].view(n, h, w, ld)[..., :c] = t
    return buf.to(dev)


def rnd(g, shape, scale=1.0, shift=0.0):
    return torch.from_numpy((g.standard_normal(shape) * scale + shift).astype(np.float32))


def test_gate_form_runs_exact_fp32(dev):
    """vt_conv2d_gate (the Fusion gate's mask conv on the thin-output kernel, which also writes f_E * m_E) with dtype
    VT_F32X3: the thin kernels have no f32x3 instance -- mask and fem are the bits of the VT_F32 call.  N = 2, 20 x 19, one K
    step of channels: the smallest shape of tests/test_fusion_gate_fem.py."""
    n, h, w, c = 2, 20, 19, 16
    g = np.random.default_rng(1016)
    fg, fe = rnd(g, (n, h, w, c)).to(dev), strided(rnd(g, (n, h, w, c)), c + 16, dev)
    sc, sh = rnd(g, (n, 2 * c), 0.5, 1.0).to(dev), rnd(g, (n, 2 * c), 0.3).to(dev)
    wt, bias = rnd(g, (1, 9, 2 * c), 1.0 / np.sqrt(18 * c)).to(dev), torch.tensor([0.05]).to(dev)
    res = {}
    for dt in (K.VT_F32X3, K.VT_F32):
        mask, fem = nan_buf(n * h * w, dev), nan_buf(n * h * w * (c + 8), dev)
        kw = dict(src0=fg, c0=c, ld0=c, src1=fe, c1=c, ld1=c + 16, in_scale=sc, in_shift=sh, in_absdiff=1, n=n, h=h, w=w,
                  out_h=h, out_w=w, weight=wt, cout=1, kh=3, kw=3, pad=1, bias=bias, act=K.ACT_RELU_TANH, out=mask, ld_out=0,
                  out_layout=K.OUT_NCHW, out_dtype=K.VT_F32, dtype=dt)
        code = _lib.lib().vt_conv2d_tile(C.byref(K.make_conv_desc(**kw)))
        assert code // P == 6, code
        K.conv2d_gate(fem, c + 8, **kw)
        rows = fem[:-TAIL].view(n, h, w, c + 8)
        assert bool(torch.isnan(mask[-TAIL:]).all()) and bool(torch.isnan(fem[-TAIL:]).all()) and bool(torch.isnan(rows[..., c:]).all())
        assert bool(torch.isfinite(mask[:-TAIL]).all()) and bool(torch.isfinite(rows[..., :c]).all())
        res[dt] = (mask[:-TAIL].cpu(), rows[..., :c].cpu().contiguous())
    report(SimpleNamespace(name="vt_conv2d_gate (thin kernel, no f32x3 instance)"), dev, code, "exact fp32 bits")
    assert float(res[K.VT_F32][0].max()) > 0
    assert same_bits(res[K.VT_F32X3][0], res[K.VT_F32][0]) and same_bits(res[K.VT_F32X3][1], res[K.VT_F32][1])


def test_hdr_form_runs_exact_fp32(dev):
    """vt_conv2d_hdr (fusion_skip with the skip planes as a K header) with dtype VT_F32X3: the bits of the VT_F32 call."""
    n, h, w, c, hdr, cout = 2, 20, 19, 16, 64, 3
    g = np.random.default_rng(2016)
    fem = strided(rnd(g, (n, h, w, c)), c + 16, dev)
    skip = rnd(g, (n, 3, h, w)).to(dev)
    wt, bias = rnd(g, (cout, 9, c + hdr), 1.0 / np.sqrt(9 * (c + 3))).to(dev), rnd(g, (cout,), 0.1).to(dev)
    res = {}
    for dt in (K.VT_F32X3, K.VT_F32):
        out = nan_buf(n * cout * h * w, dev)
        K.conv2d_hdr(skip, 3, hdr, src0=fem, c0=c, ld0=c + 16, n=n, h=h, w=w, out_h=h, out_w=w, weight=wt, cout=cout, kh=3, kw=3,
                     pad=1, bias=bias, out=out, ld_out=0, out_layout=K.OUT_NCHW, out_dtype=K.VT_F32, dtype=dt)
        assert bool(torch.isnan(out[-TAIL:]).all()) and bool(torch.isfinite(out[:-TAIL]).all())
        res[dt] = out[:-TAIL].cpu()
    report(SimpleNamespace(name="vt_conv2d_hdr (thin kernel, no f32x3 instance)"), dev, 6 * P, "exact fp32 bits")
    assert float(res[K.VT_F32].abs().max()) > 0.1 and same_bits(res[K.VT_F32X3], res[K.VT_F32])


def torgb_problem(n, hh, ww, cin, cout, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, cin, hh, ww)).astype(np.float32)
    w = (g.standard_normal((cout, cin, 3, 3)) / math.sqrt(9 * cin)).astype(np.float32)
    b = g.standard_normal(cout).astype(np.float32)
    wr = (g.standard_normal((3, cout, 1, 1)) / math.sqrt(cout)).astype(np.float32)
    br = g.standard_normal(3).astype(np.float32)
    skip = g.standard_normal((n, 3, hh, ww)).astype(np.float32)
    return x, w, b, wr, br, skip


def test_rgbup_form_is_refused(dev):
    """vt_conv2d_rgbup (Upsample(skip) in the fused-ToRGB epilogue) exists on the persistent 32 -> 32 kernel and the
    weights-resident patch form, both 16-bit only: with fp32 tensors -- VT_F32X3 as VT_F32 -- it is VT_ERR_UNSUPPORTED and
    launches nothing.  N = 2, 32 -> 32 at 40 x 56: the smallest shape of tests/test_rgb_skip_fold.py."""
    n, hh, ww, c = 2, 40, 56, 32
    x, w, b, wr, br, _ = torgb_problem(n, hh, ww, c, c, 11)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt, wp, wrp = K.nchw_to_nhwc(dv(x), torch.float32), K.pack_conv_weight(dv(w)), K.pack_conv_weight(dv(wr))
    lo = rnd(np.random.default_rng(3), (n, 3, hh // 2, ww // 2)).to(dev)
    fir, bt, brt = dv(FIR_STD), dv(b), dv(br)
    for dt in (K.VT_F32X3, K.VT_F32):
        out, rgb = nan_buf(n * hh * ww * c, dev), nan_buf(n * 3 * hh * ww, dev)
        d = K.make_conv_desc(src0=xt, c0=c, ld0=c, n=n, h=hh, w=ww, out_h=hh, out_w=ww, weight=wp, cout=c, kh=3, kw=3, pad=1,
                             bias=bt, act=L, gain=2 ** 0.5, out=out, ld_out=c, dtype=dt, rgb_weight=wrp, rgb_bias=brt,
                             rgb_resid=rgb, rgb_out=rgb)
        rc = _lib.lib().vt_conv2d_rgbup(C.byref(d), lo.data_ptr(), fir.data_ptr(), K._stream(out))
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert rc == UNSUPPORTED, (dt, rc)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(rgb).all()), "a refused call launched something"
    report(SimpleNamespace(name="vt_conv2d_rgbup (16-bit kernels only)"), dev, 0, "refused")


@pytest.mark.parametrize("what,cin,cout,H,W,hint,kind", [("patch 128x64", 64, 64, 9, 40, P + 1000000 + 128064, 1),
                                                         ("1d 128x128", 64, 128, 12, 20, 2 * P + 1000000 + 128128, 2)])
def test_fused_torgb(dev, what, cin, cout, H, W, hint, kind):
    """A conv with the fused ToRGB (rgb_weight) is accepted in f32x3: the activation against the three-term model, and the
    planes -- W_rgb . act(conv) + bias + skip, formed by the f32x3 instances on the vector ALUs in fp32 from the finished
    values, NOT split -- against the float64 ToRGB of the model's activation, bound 4 tau S with S = |W_rgb| . S_act and tau
    from the float32 evaluation of the same chain."""
    n = 2
    x, w, b, wr, br, skip = torgb_problem(n, H, W, cin, cout, 12 + cout)
    c = case(f"fused ToRGB, {what}", n, cin, H, W, cout, act=L, hint=hint, kind=kind)
    model, exact, S, tau = reference(c, x, w, b, None)
    f64, f32 = torch.float64, torch.float32
    rgb_of = lambda y, dt: F.conv2d(y, _t(wr, dt)) + _t(br, dt).view(1, 3, 1, 1) + _t(skip, dt)
    rgb_model = rgb_of(model, f64)
    rgb32 = rgb_of(epilogue(c, three_terms(c, x, w, f32), b, None, f32), f32)
    S_rgb = F.conv2d(S, _t(np.abs(wr), f64))
    tau_rgb = float(((rgb32.double() - rgb_model).abs() / S_rgb).max())
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt, wp, wrp = K.nchw_to_nhwc(dv(x), torch.float32), K.pack_conv_weight(dv(w)), K.pack_conv_weight(dv(wr))
    res = {}
    bt, brt = dv(b), dv(br)
    for dt in (K.VT_F32X3, K.VT_F32):
        out = nan_buf(n * H * W * cout, dev)
        rgb = torch.cat([dv(skip).reshape(-1), torch.full((TAIL,), float("nan"), device=dev)])
        d = K.make_conv_desc(src0=xt, c0=cin, ld0=cin, n=n, h=H, w=W, out_h=H, out_w=W, weight=wp, cout=cout, kh=3, kw=3, pad=1,
                             bias=bt, act=L, gain=2 ** 0.5, out=out, ld_out=cout, dtype=dt, tile_hint=hint, rgb_weight=wrp,
                             rgb_bias=brt, rgb_resid=rgb, rgb_out=rgb)
        code = _lib.lib().vt_conv2d_tile(C.byref(d))
        assert code // P == kind and code % 1000000 == hint % 1000000, code
        _lib.check(_lib.lib().vt_conv2d(C.byref(d), K._stream(out)), "vt_conv2d")
        assert bool(torch.isnan(out[-TAIL:]).all()) and bool(torch.isnan(rgb[-TAIL:]).all()), "tail written"
        res[dt] = (out[:-TAIL].view(n, H, W, cout).permute(0, 3, 1, 2).cpu().contiguous(), rgb[:-TAIL].view(n, 3, H, W).cpu())
    assert not same_bits(res[K.VT_F32X3][0], res[K.VT_F32][0]), "the f32x3 instance did not run"
    bound_check(c.name + ": activation", dev, code, res[K.VT_F32X3][0], model, S, tau)
    bound_check(c.name + ": planes", dev, code, res[K.VT_F32X3][1], rgb_model, S_rgb, tau_rgb)
