"""fp16 compute precision of the engine (VToonifyEngine(dtype=torch.float16), VToonify(compute_dtype=torch.float16),
VTOONIFY_AMD_DTYPE=fp16, --precision fp16): fp16 activations and weights, fp32 accumulation, statistics, demodulation, style
path and planar RGB skip path, on the kernel families, tiles and plans of the bf16 engine.

Tolerances:
  * single convolutions: against float64 on the fp16-ROUNDED operands, so only the fp32 accumulation order and the rounding of
    the output remain: |y - ref| <= 2e-5 x max|ref| (fp32 slack) + half an fp16 ulp of |ref| (2^-11 relative).  The output
    tensor has NaN-filled slack channels and a NaN-filled tail: they must keep the sentinel.
  * forms that round an intermediate inside the kernel (AdaIN loader, fused ToRGB operand, the up-sampling z tile / rows):
    the reference rounds the same intermediate to fp16; see FLIP_FRAC below.  Rounding it to bf16 instead fails these.
  * the kernel families' own suites (tests/test_ops.py), rerun on fp16 operands: extra coverage at their 16-bit bars only.
  * end to end, against the REFERENCE's goldens (tests/golden/e2e_*.npz) and the fp32 oracle: PSNR >= FP16_PSNR and at least
    FP16_GAIN_DB above the bf16 engine on the same inputs, q99.9 of |error| <= FP16_Q999 x max|ref|, max-rel <= FP16_TOL.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, load_keys, psnr, rel_err
from vtoonify_amd import kernels as K
from vtoonify_amd import synth
from vtoonify_amd.engine import VToonifyEngine

# measured on MI355X: PSNR 69.5-78.6 dB, 18-21 dB above bf16, q99.9 <= 3.2e-3, max-rel <= 4.4e-3
FP16_PSNR, FP16_GAIN_DB, FP16_Q999, FP16_TOL = 63.0, 10.0, 5e-3, 9e-3
BB = {"D": "dualstylegan", "T": "toonify"}
GEOMS = [(256, 256), (144, 256), (384, 384), (360, 400)]   # every BASELINE frame geometry
_sd_cache = {}


def _sd(tag):
    if tag not in _sd_cache:
        _sd_cache.clear()
        _sd_cache[tag] = synth.synth_state_dict(load_keys(tag), 0)
    return _sd_cache[tag]


def _engine(tag, dtype, dev, **kw):
    return VToonifyEngine({k: v.to(dev) for k, v in _sd(tag).items()}, BB[tag], 256, dtype, dev, **kw)


def _metrics(y, ref):
    y = np.asarray(y, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    scale = max(float(np.abs(ref).max()), 1e-30)
    return (rel_err(y, ref), psnr(y, ref, float(ref.max() - ref.min())),
            float(np.quantile(np.abs(y - ref), 0.999) / scale))


def _check_fp16(y, ref, what):
    e, p, q = _metrics(y.float().cpu().numpy() if isinstance(y, torch.Tensor) else y, ref)
    print(f"[parity] {what} fp16: max-rel {e:.3e}, PSNR {p:.1f} dB, q99.9 {q:.2e}")
    assert e <= FP16_TOL and p >= FP16_PSNR and q <= FP16_Q999, f"{what}: rel {e:.2e}, q99.9 {q:.2e}, psnr {p:.1f} dB"
    return p


def _tiles(eng, B, H, W):
    """(kind, bm, bn, splitk) of every conv of the frame plan, from the host query vt_conv2d_tile."""
    plan = eng._build_plan(B, H, W, True, True)   # descriptors and buffers only: nothing is launched
    out = []
    for d, info, _, _ in plan.convs:
        code = eng.lib.vt_conv2d_tile(ctypes.byref(d))
        assert code >= 0
        out.append((info["sig"], code // 100000000, (code // 1000) % 1000, code % 1000, (code // 1000000) % 100))
    return out


# ---------------------------------------------------------------------------------------------------------------- plans
@pytest.mark.parametrize("tag", ["D", "T"])
def test_fp16_plans_equal_bf16_plans(monkeypatch, tag):
    """Every conv of the fp16 frame gets the kernel family, tile and K split of the bf16 frame, at every BASELINE geometry,
    for one frame and for four, with and without VT_BATCH_EXACT=1 -- and none of the specialised families is missing."""
    from emu import build_emu
    from vtoonify_amd import _lib
    _lib.use_library(build_emu.build())
    dev = torch.device("cpu")
    e16, eb = _engine(tag, torch.float16, dev), _engine(tag, torch.bfloat16, dev)
    for exact in ("0", "1"):
        monkeypatch.setenv("VT_BATCH_EXACT", exact)
        for (H, W) in GEOMS:
            for B in (1, 4):
                p16, pb = _tiles(e16, B, H, W), _tiles(eb, B, H, W)
                assert p16 == pb, (exact, H, W, B, [(a, b) for a, b in zip(p16, pb) if a != b][:4])
                kinds = {k for _, k, _, _, _ in p16}
                assert kinds - {0, 2}, "the fp16 plan runs no specialised family"


# ------------------------------------------------------------------------------------------------- single convolutions
def _conv_fp16(dev, N, Cin, H, W, Cout, k, stride=1, pad=1, dil=1, act=K.ACT_LRELU, resid=False, hint=0, stream=False,
               ws=False, expect_kind=None, seed=0):
    """One fp16 conv with NaN sentinels around its output, against float64 on the rounded operands."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (g.standard_normal((Cout, Cin, k, k)) / math.sqrt(Cin * k * k)).astype(np.float32)
    b = g.standard_normal(Cout).astype(np.float32)
    cpad = (Cin + 7) // 8 * 8
    xt = K.nchw_to_nhwc(torch.from_numpy(x).to(dev), torch.float16)
    wp = K.pack_conv_weight(torch.from_numpy(w).to(dev), cin_dst=cpad, out_dtype=torch.float16)
    Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    xq = xt.double().cpu().permute(0, 3, 1, 2)[:, :Cin]
    wq = wp.double().cpu().reshape(Cout, k, k, cpad)[..., :Cin].permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(xq, wq, torch.from_numpy(b).double(), stride, pad, dil)
    gain = 1.0
    if act == K.ACT_LRELU:
        ref, gain = torch.where(ref > 0, ref, 0.2 * ref) * math.sqrt(2), math.sqrt(2)
    ldo = (Cout + 7) // 8 * 8 + 8                      # 8+ slack channels per pixel
    slack = 64                                         # and a tail behind the last pixel
    buf = torch.full((N * Ho * Wo * ldo + slack,), float("nan"), dtype=torch.float16, device=dev)
    out = buf[:N * Ho * Wo * ldo].view(N, Ho, Wo, ldo)
    r = None
    if resid:
        rn = g.standard_normal((N, Cout, Ho, Wo)).astype(np.float32)
        r = K.nchw_to_nhwc(torch.from_numpy(rn).to(dev), torch.float16, ld_out=ldo)
        ref = ref * 0.5 + 0.25 * r.double().cpu().permute(0, 3, 1, 2)[:, :Cout]
    common = dict(src0=xt, c0=cpad, ld0=cpad, n=N, h=H, w=W, out_h=Ho, out_w=Wo, weight=wp, cout=Cout, kh=k, kw=k,
                  stride=stride, pad=pad, dil=dil, bias=torch.from_numpy(b).to(dev), act=act, gain=gain, dtype=K.VT_F16,
                  tile_hint=hint, alpha=0.5 if resid else 1.0, beta=0.25 if resid else 0.0, out=out, ld_out=ldo,
                  resid=r, ld_res=ldo)
    if stream:
        common["weight_stream"] = K.conv_weight_stream(wp)
        assert common["weight_stream"] is not None
    if ws:
        common["splitk_ws"] = torch.zeros(8 << 20, dtype=torch.float32, device=dev)
    if expect_kind is not None:
        from vtoonify_amd import _lib
        d = K.make_conv_desc(**common)
        code = _lib.lib().vt_conv2d_tile(ctypes.byref(d))
        assert code // 100000000 == expect_kind, f"kernel kind {code}"
    K.conv2d(**common)
    y = out.double().cpu().permute(0, 3, 1, 2)[:, :Cout]
    assert torch.isnan(out[..., Cout:].float()).all(), "slack channels written"
    assert torch.isnan(buf[N * Ho * Wo * ldo:].float()).all(), "tail written"
    assert torch.isfinite(y).all()
    bound = 2e-5 * float(ref.abs().max()) + 2.0 ** -11 * ref.abs() + 1e-7
    bad = (y - ref).abs() > bound
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} outside fp32 slack + half an fp16 ulp"


P = 100000000
_FAMILIES = [   # (what, args, kwargs): ragged tile counts throughout
    ("generic register-staged", (1, 22, 13, 9, 32, 3), dict(hint=1000000000 + 128032, expect_kind=0)),
    ("generic direct-to-LDS, split-K", (1, 128, 9, 7, 64, 3), dict(hint=4 * 1000000 + 64064, ws=True, expect_kind=2)),
    ("c32 persistent", (2, 32, 21, 34, 32, 3), dict(expect_kind=3)),
    ("c32 persistent, 32 -> 128", (1, 32, 19, 23, 128, 3), dict(expect_kind=3)),
    ("patch 128x64", (1, 64, 19, 21, 64, 3), dict(hint=P + 128064, expect_kind=1)),
    ("patch 256x64 pipelined", (1, 64, 37, 21, 64, 3), dict(hint=P + 256064, expect_kind=1)),
    ("patch 256x128 pipelined", (1, 128, 21, 35, 128, 3), dict(hint=P + 256128, resid=True, expect_kind=1)),
    ("patch 256x32 chunk", (1, 128, 19, 21, 32, 3), dict(hint=P + 256032, expect_kind=1)),
    ("patch 256x32 dil 2", (1, 128, 19, 21, 32, 3), dict(hint=P + 256032, pad=2, dil=2, expect_kind=1)),
    ("patch 128x128 split-K", (1, 128, 11, 13, 128, 3), dict(hint=P + 2 * 1000000 + 128128, ws=True, expect_kind=1)),
    ("stride-2 by parity", (2, 64, 34, 46, 64, 3), dict(stride=2, hint=7 * P + 256064, expect_kind=7)),
    ("stride-2 by parity, 32-channel tiles", (1, 128, 40, 72, 40, 3), dict(stride=2, hint=7 * P + 256032, resid=True,
                                                                             expect_kind=7)),
    ("whole-K", (1, 512, 9, 11, 136, 3), dict(stream=True, resid=True, expect_kind=4)),
    ("whole-K dil 2", (1, 512, 9, 11, 40, 3), dict(stream=True, pad=2, dil=2, hint=4 * P, expect_kind=4)),
    ("whole-K weight-stationary", (4, 512, 9, 11, 136, 3), dict(stream=True, resid=True, expect_kind=8,
                                                                 env={"VT_FULLKW_MIN_G": "1"})),
    ("patch weights resident", (1, 64, 40, 37, 64, 3), dict(hint=P + 1000000 + 256064, expect_kind=1,
                                                             env={"VT_PATCHW_WGS": "2"})),
    ("patch persistent 256x128", (1, 128, 35, 37, 128, 3), dict(hint=P + 1000000 + 256128, expect_kind=1,
                                                                 env={"VT_PATCHW_WGS": "2"})),
    ("patch persistent 256x64", (1, 128, 35, 37, 64, 3), dict(hint=P + 1000000 + 256064, expect_kind=1,
                                                               env={"VT_PATCHW_WGS": "3"})),
]


@pytest.mark.parametrize("what,args,kw", _FAMILIES, ids=[f[0] for f in _FAMILIES])
def test_fp16_conv_families_vs_float64(dev, monkeypatch, what, args, kw):
    kw = dict(kw)
    for k, v in kw.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    _conv_fp16(dev, *args, **kw)


# the families' own suites (edge shapes, fused ToRGB, statistics records, up_fir forms, in_absdiff + AdaIN loader, split-K)
# on fp16 operands
_OPS_SUITES = ["test_conv_shapes", "test_conv_thin_kernel", "test_conv_thin_gate_prologue",
               "test_conv_direct_to_lds_and_patch_kernels", "test_conv_fused_torgb", "test_conv_emits_instnorm_records",
               "test_conv_patch_pipelined_dilated", "test_conv_patch_pipelined_equals_per_tap", "test_conv_transpose_by_parity",
               "test_styled_conv_golden", "test_instnorm_adain_fusion_pack", "test_instnorm_plane_one_launch",
               "test_conv_whole_k_kernel", "test_conv_whole_k_adain_chain", "test_conv_weight_stationary_equals_whole_k",
               "test_conv_transpose_blur_persistent_form", "test_conv_transpose_blur_kernel"]


@pytest.mark.parametrize("name", _OPS_SUITES)
def test_fp16_family_suites(dev, monkeypatch, name):
    import inspect
    import test_ops
    f = getattr(test_ops, name)
    kw = {"dtype": torch.float16}
    if "monkeypatch" in inspect.signature(f).parameters:
        kw["monkeypatch"] = monkeypatch
    f(dev, **kw)


def test_fp16_upblur_rows_form(dev, monkeypatch):
    """The strip-marching up-sampling form (conv_upblur_rows.hpp, plan kind 9) in fp16, forced on small images: against float64
    conv_transpose2d -> blur -> bias + LeakyReLU on the rounded operands (the z rows are rounded to fp16 inside the kernel: a few
    fp16 ulps), against the tile kernel, and with a FIR whose taps are not fp16 numbers (remainder products)."""
    from vtoonify_amd import _lib
    g = np.random.default_rng(77)
    k1 = np.array([1, 3, 3, 1], np.float64)
    fir_std = np.outer(k1, k1) / 64.0 * 4.0
    fir_odd = np.outer(k1, np.array([0.9, 3.1, 2.7, 1.3])) / 64.0 * 4.0
    for N, cin, H, W, cout, fir, wgs in [(2, 64, 21, 19, 32, fir_std, "3"), (1, 128, 13, 31, 40, fir_std, "2"),
                                         (1, 64, 9, 45, 64, fir_odd, "1")]:
        x = g.standard_normal((N, cin, H, W)).astype(np.float32)
        w = (g.standard_normal((cout, cin, 3, 3)) / math.sqrt(cin * 9)).astype(np.float32)
        b = g.standard_normal(cout).astype(np.float32)
        xt = K.nchw_to_nhwc(torch.from_numpy(x).to(dev), torch.float16)
        wp = K.pack_conv_weight(torch.from_numpy(w).to(dev), out_dtype=torch.float16)
        firt = torch.from_numpy(fir.astype(np.float32)).to(dev)
        xq = xt.double().cpu().permute(0, 3, 1, 2)
        wq = wp.double().cpu().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
        z = torch.nn.functional.conv_transpose2d(xq, wq.transpose(0, 1), stride=2)
        kf = torch.from_numpy(fir.astype(np.float32)).double().flip(0, 1)[None, None].repeat(cout, 1, 1, 1)
        zb = torch.nn.functional.conv2d(torch.nn.functional.pad(z, (1, 1, 1, 1)), kf, groups=cout)
        ref = zb + torch.from_numpy(b).double()[None, :, None, None]
        ref = torch.where(ref > 0, ref, 0.2 * ref) * math.sqrt(2)

        def run(rows):
            monkeypatch.setenv("VT_UPBLUR_ROWS", rows)
            monkeypatch.setenv("VT_UPBLUR_WGS", wgs)
            out = torch.full((N, 2 * H, 2 * W, cout + 8), float("nan"), dtype=torch.float16, device=dev)
            common = dict(src0=xt, c0=cin, ld0=cin, n=N, h=H, w=W, out_h=2 * H, out_w=2 * W, weight=wp, cout=cout, kh=3,
                          kw=3, bias=torch.from_numpy(b).to(dev), act=K.ACT_LRELU, gain=2 ** 0.5, out=out, ld_out=cout + 8,
                          dtype=K.VT_F16, up_fir=firt, tile_hint=32)
            code = _lib.lib().vt_conv2d_tile(ctypes.byref(K.make_conv_desc(**common)))
            assert code // 100000000 == (9 if rows == "1" else 5), code
            K.conv2d(**common)
            assert torch.isnan(out[..., cout:].float()).all(), "slack channels written"
            return out[..., :cout].double().cpu().permute(0, 3, 1, 2)
        y_rows, y_tile = run("1"), run("0")
        scale = float(ref.abs().max())
        assert float((y_rows - ref).abs().max()) <= 4e-3 * scale, (N, cin, H, W, cout)
        assert float((y_rows - y_tile).abs().max()) <= 4e-3 * scale, (N, cin, H, W, cout)
    monkeypatch.delenv("VT_UPBLUR_ROWS")


# ------------------------------------------------------------------------------------------------------- glue kernels
def test_fp16_modulate_weight_batch(dev):
    """vt_modulate_weight_batch with out_dtype = VT_F16 (modulation, demodulation and the FIR fold in fp32, rounded once at the
    store): every element is the fp32 launch's value rounded once to fp16, including the polyphase FIR items."""
    from vtoonify_amd import _lib
    g = np.random.default_rng(11)
    fir = torch.from_numpy((np.outer([1, 3, 3, 1], [1, 3, 3, 1]) / 64.0 * 4.0).astype(np.float32)).to(dev)
    specs = [(64, 32, 3, 1, 0), (3, 64, 1, 0, 0), (40, 24, 3, 1, 1), (16, 64, 3, 1, 0)]
    outs = {}
    for dt, tdt in ((K.VT_F32, torch.float32), (K.VT_F16, torch.float16)):
        keep, items = [], []
        for i, (cout, cin, k, demod, use_fir) in enumerate(specs):
            gg = np.random.default_rng(100 + i)
            w = torch.from_numpy(gg.standard_normal((cout, cin, k, k)).astype(np.float32)).to(dev)
            sv = torch.from_numpy((gg.standard_normal(cin) + 1.0).astype(np.float32)).to(dev)
            phases = 4 if use_fir else 1
            out = torch.full((cout * phases * 9 * cin + 64,), float("nan"), dtype=tdt, device=dev)
            keep += [out, w, sv]
            items.append(_lib.ModulateItem(out.data_ptr(), w.data_ptr(), sv.data_ptr(), fir.data_ptr() if use_fir else 0,
                                           cout, cin, k, demod, 1.0 / math.sqrt(cin * k * k), 0))
        arr = (_lib.ModulateItem * len(items))(*items)
        rc = _lib.lib().vt_modulate_weight_batch(arr, len(items), dt, K._stream(fir))
        assert rc == 0, _lib.lib().vt_last_error()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        outs[dt] = [keep[3 * i].cpu() for i in range(len(specs))]
    del g
    for o32, o16 in zip(outs[K.VT_F32], outs[K.VT_F16]):
        live = ~torch.isnan(o32)
        assert torch.equal(torch.isnan(o16), ~live), "fp16 launch wrote other elements than the fp32 one"
        a, r = o16[live].double(), o32[live].double()
        # one rounding to fp16 of the fp32 value (the instances may order the fp32 arithmetic differently: 1e-6 of slack)
        assert bool(((a - r).abs() <= 2.0 ** -11 * r.abs() + 1e-6 * float(r.abs().max())).all())


def test_fp16_affine_and_fusion_pack_vs_float64(dev):
    """vt_affine_apply (with the |x - other| half) and vt_fusion_pack in fp16, per element against float64."""
    from vtoonify_amd import _lib
    lib = _lib.lib()
    g = np.random.default_rng(3)
    n, hw, c = 2, 37, 24
    x = torch.from_numpy(g.standard_normal((n, hw, c)).astype(np.float32)).half().to(dev)
    o = torch.from_numpy(g.standard_normal((n, hw, c)).astype(np.float32)).half().to(dev)
    sc = torch.from_numpy(g.standard_normal((n, 2 * c)).astype(np.float32)).to(dev)
    sh = torch.from_numpy(g.standard_normal((n, 2 * c)).astype(np.float32)).to(dev)
    out = torch.full((n, hw, 2 * c + 8), float("nan"), dtype=torch.float16, device=dev)
    st = torch.cuda.current_stream().cuda_stream if dev.type == "cuda" else 0
    rc = lib.vt_affine_apply(ctypes.c_void_p(out.data_ptr()), 2 * c + 8, ctypes.c_void_p(x.data_ptr()), c,
                             ctypes.c_void_p(o.data_ptr()), c, ctypes.c_void_p(sc.data_ptr()), ctypes.c_void_p(sh.data_ptr()),
                             n, hw, c, K.VT_F16, ctypes.c_void_p(st))
    assert rc == 0, lib.vt_last_error()
    xd, od = x.double().cpu(), o.double().cpu()
    cat = torch.cat([xd, (xd - od).abs()], -1)
    ref = cat * sc.double().cpu()[:, None, :] + sh.double().cpu()[:, None, :]
    y = out[..., :2 * c].double().cpu()
    assert torch.isnan(out[..., 2 * c:].float()).all()
    assert ((y - ref).abs() <= 2e-6 * ref.abs().max() + 2.0 ** -11 * ref.abs()).all()
    # fusion_pack: [skip(3) | pad | f_E * mask] rows of header 8 + c channels
    fe = torch.from_numpy(g.standard_normal((n, hw, c)).astype(np.float32)).half().to(dev)
    mask = torch.from_numpy(g.random((n, 1, hw)).astype(np.float32)).to(dev)
    skip = torch.from_numpy(g.standard_normal((n, 3, hw)).astype(np.float32)).to(dev)
    pk = torch.full((n, hw, 8 + c), float("nan"), dtype=torch.float16, device=dev)
    rc = lib.vt_fusion_pack(ctypes.c_void_p(pk.data_ptr()), 8 + c, ctypes.c_void_p(fe.data_ptr()), c,
                            ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(skip.data_ptr()), n, hw, c, K.VT_F16,
                            ctypes.c_void_p(st))
    assert rc == 0, lib.vt_last_error()
    pkd = pk.double().cpu()
    ref_f = fe.double().cpu() * mask.double().cpu().permute(0, 2, 1)
    assert ((pkd[..., 8:] - ref_f).abs() <= 2.0 ** -11 * ref_f.abs() + 1e-7).all()
    ref_s = skip.double().cpu().permute(0, 2, 1)
    assert ((pkd[..., :3] - ref_s).abs() <= 2.0 ** -11 * ref_s.abs() + 1e-7).all()


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("tag", ["D", "T"])
def test_fp16_golden_vs_reference(dev, tag):
    """Both golden frames of the reference (d_s keys and the per-sample-style batch) in fp16: the fp16 bars, and at least
    FP16_GAIN_DB above the bf16 engine on the same inputs."""
    d, _ = load_golden(f"e2e_{tag}.npz")
    x, s = torch.from_numpy(d["x"]).to(dev), torch.from_numpy(d["style"]).to(dev)
    keys = [k for k in d if k.startswith("y_ds")][:1 if dev.type == "cpu" else None]
    x2, s2 = torch.from_numpy(d["x2"]).to(dev), torch.from_numpy(d["style2"]).to(dev)
    e16 = _engine(tag, torch.float16, dev)
    assert e16.precision == "fp16"
    ys = {k: e16.forward(x, s, float(k[4:])).float().cpu().numpy() for k in keys}
    ys["y2_ds0.75"] = e16.forward(x2, s2, 0.75).float().cpu().numpy()
    kinds = {info["kernel"] for _, _, info in e16.frame_ops(next(reversed(e16._plans.values())))
             if isinstance(info, dict) and info["kernel"].startswith("conv_") and "<" in info["kernel"]}
    assert kinds and all("<f16," in k for k in kinds), kinds
    del e16
    eb = _engine(tag, torch.bfloat16, dev)
    for k, y in ys.items():
        p16 = _check_fp16(y, d[k], f"{tag} {k}")
        yb = (eb.forward(x, s, float(k[4:])) if k.startswith("y_ds") else eb.forward(x2, s2, 0.75)).float().cpu().numpy()
        pb = _metrics(yb, d[k])[1]
        assert p16 >= pb + FP16_GAIN_DB, f"{tag} {k}: fp16 {p16:.1f} dB, bf16 {pb:.1f} dB"


# ------------------------------------------------------------------------------------------------------------- surface
def test_fp16_public_surface(monkeypatch):
    from vtoonify_amd.vtoonify import VToonify
    assert VToonify(compute_dtype=torch.float16).precision == "fp16"
    for env in ("fp16", "float16", "FP16"):
        monkeypatch.setenv("VTOONIFY_AMD_DTYPE", env)
        m = VToonify()
        assert m.precision == "fp16" and m.compute_dtype == torch.float16
    monkeypatch.setenv("VTOONIFY_AMD_DTYPE", "half")
    with pytest.raises(ValueError):
        VToonify()


def test_fp16_cli_video_within_the_bar_of_fp32_exact(dev, tmp_path):
    """tools/style_transfer_amd.py --precision fp16 on a small .npy clip writes the video, and it is within the fp16 bar of
    the --precision fp32_exact video of the same clip (uint8 frames: PSNR over 255 levels, at most 2 levels apart)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import style_transfer_amd as cli
    from test_style_transfer_cli import _args, _clip
    _clip(tmp_path, n=3)
    device = "cpu" if dev.type == "cpu" else "cuda:0"
    vids = {}
    for prec in ("fp16", "fp32_exact"):
        rep = cli.main(_args(tmp_path, tmp_path / prec, extra=("--precision", prec)), device=device)
        assert rep["frames"] == 3
        vids[prec] = np.load(rep["output"])
    a, b = vids["fp16"].astype(np.int32), vids["fp32_exact"].astype(np.int32)
    assert a.shape == b.shape == (3, 64, 96, 3)
    diff = np.abs(a - b)
    frac = float((diff > 0).mean())
    print(f"[cli] fp16 vs fp32_exact: {frac:.4f} of uint8 values differ, max {int(diff.max())}, "
          f"PSNR {psnr(a, b, 255.0):.1f} dB")
    assert int(diff.max()) <= 2 and psnr(a, b, 255.0) >= 45.0


# --------------------------------------------------------------------------------------------------- GPU, full size
def _oracle(tag, x, s):
    from oracle import vtoonify_oracle as O
    old = O.set_backend("torch")
    try:
        sdn = synth.to_numpy_sd(_sd(tag))
        return np.concatenate([O.vtoonify_forward(sdn, x[i:i + 1].numpy(), s.numpy(), 0.5, BB[tag])
                               for i in range(x.shape[0])], 0)
    finally:
        O.set_backend(old)


def _gpu():
    from vtoonify_amd import _lib
    _lib.use_library(_lib.DEFAULT_LIB)
    assert not _lib.is_emulation()
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("tag,hw", [("D", (256, 256)), ("T", (144, 256)), ("T", (256, 256)), ("D", (384, 384)),
                                    ("D", (360, 400))])
def test_fp16_full_size_vs_oracle(tag, hw):
    """Every BASELINE frame geometry (the configurations of test_engine.py::test_full_size_fp32_vs_oracle) in fp16 against
    the fp32 oracle, and FP16_GAIN_DB above bf16 on the same frame."""
    dev = _gpu()
    x = synth.synth_frames(1, hw[0], hw[1], seed=99)
    s = synth.synth_style(seed=17)
    ref = _oracle(tag, x, s)
    y = _engine(tag, torch.float16, dev).forward(x.to(dev), s.to(dev), 0.5)
    assert tuple(y.shape) == (1, 3, 4 * hw[0], 4 * hw[1])
    p16 = _check_fp16(y, ref, f"{tag} {hw}")
    pb = _metrics(_engine(tag, torch.bfloat16, dev).forward(x.to(dev), s.to(dev), 0.5).float().cpu().numpy(), ref)[1]
    print(f"[parity] {tag} {hw}: fp16 {p16:.1f} dB, bf16 {pb:.1f} dB")
    assert p16 >= pb + FP16_GAIN_DB


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(256, 256), (144, 200)])
def test_fp16_headline_batch4(monkeypatch, hw):
    """The headline step in fp16 (D, 4 frames per call, the batch-aware plans): every frame against the oracle; hipGraph replay
    bitwise equal to eager launches; under VT_BATCH_EXACT=1 a frame inside the batch bitwise equal to the frame alone."""
    dev = _gpu()
    x = synth.synth_frames(4, hw[0], hw[1], seed=77)
    s = synth.synth_style(seed=17)
    ref = _oracle("D", x, s)
    xd, sd4 = x.to(dev), s.to(dev).repeat(4, 1, 1)
    eng = _engine("D", torch.float16, dev)
    y = eng.forward(xd, sd4, 0.5, use_graph=False).clone()
    _check_fp16(y, ref, f"D 4x{hw}")
    for _ in range(2):   # capture, then replay
        yg = eng.forward(xd, sd4, 0.5, use_graph=True).clone()
        assert torch.equal(yg, y), "graph replay differs from eager launches"
    monkeypatch.setenv("VT_BATCH_EXACT", "1")
    eng_x = _engine("D", torch.float16, dev)
    yb = eng_x.forward(xd, sd4, 0.5).clone()
    alone = torch.cat([eng_x.forward(xd[i:i + 1].contiguous(), s.to(dev), 0.5).clone() for i in range(4)])
    assert torch.equal(yb, alone)


@pytest.mark.gpu
def test_fp16_two_lanes_steady_state():
    """Two lanes (own stream and plan each) in steady state: every frame equals the same frame run alone on lane 0."""
    dev = _gpu()
    eng = _engine("D", torch.float16, dev)
    s = synth.synth_style(seed=17).to(dev)
    xs = [synth.synth_frames(2, 64, 96, seed=i).to(dev) for i in range(4)]
    want = [eng.forward(x, s, 0.5, shared_style=True, use_graph=False, lane=0).clone() for x in xs]
    streams = [torch.cuda.current_stream(dev), torch.cuda.Stream(dev)]
    got = []
    for i in range(12):
        ln = i % 2
        with torch.cuda.stream(streams[ln]):
            got.append((i % 4, eng.forward(xs[i % 4], s, 0.5, shared_style=True, use_graph=True, lane=ln).clone()))
    torch.cuda.synchronize()
    for k, y in got:
        assert torch.equal(y, want[k]), k


@pytest.mark.gpu
def test_fp16_buffers_finite_at_the_headline(capsys):
    """Range: after an fp16 frame of the headline geometry (D, 4 x 256^2) every buffer of the plan is finite, and the largest
    |value| of each fp16 buffer stays below the fp16 limit (65504).  Prints the table DESIGN.md 4.1w records."""
    dev = _gpu()
    eng = _engine("D", torch.float16, dev, style_gate=True)
    x = synth.synth_frames(4, 256, 256, seed=77).to(dev)
    s = synth.synth_style(seed=17).to(dev)
    y = eng.forward(x, s.repeat(4, 1, 1), 0.5, return_mask=True)
    torch.cuda.synchronize()
    img, masks = y
    assert torch.isfinite(img).all() and all(torch.isfinite(m).all() for m in masks)
    plan = list(eng._plans.values())[-1]
    worst = ("", 0.0)
    for name, t in plan.bufs.items():
        if t.dtype not in (torch.float16, torch.float32) or t.numel() == 0:
            continue
        m = float(t.float().abs().max())
        assert math.isfinite(m), name
        if t.dtype == torch.float16:
            print(f"[range] {name:16s} max|v| {m:10.3f}  ({m / 65504:.2e} of the fp16 limit)")
            if m > worst[1]:
                worst = (name, m)
    print(f"[range] largest: {worst[0]} {worst[1]:.3f}")
    assert worst[1] < 65504 / 16, worst
    feat, skip = eng.forward(x, s.repeat(4, 1, 1), 0.5, return_feat=True)
    assert feat.dtype == torch.float32 and torch.isfinite(feat).all() and torch.isfinite(skip).all()


# ------------------------------------------------------------------ fp16 bars for the forms that round inside the kernel
# Where a kernel rounds an intermediate to the compute type (the loader's AdaIN affine, the fused ToRGB's activation operand,
# the z tile / z rows of the up-sampling forms), the float64 reference rounds the same intermediate to fp16.  The kernel's fp32
# value of it can sit on the other side of an fp16 rounding boundary than the float64 one, so a few elements may differ by one
# fp16 ulp of that intermediate's contribution: at most FLIP_FRAC of the outputs may leave the tight bound (fp32 slack + half an
# fp16 ulp of the output), and none the loose one (tight + one fp16 ulp of every intermediate term).  Rounding the
# intermediate to bf16 instead (2^-9 relative) moves most outputs outside the tight bound.
FLIP_FRAC = 0.02
H16 = 2.0 ** -11   # half an fp16 ulp, relative


def _h(t):
    return t.half().double()


def _check_internal(y, ref, tight, loose, what):
    err = (y - ref).abs()
    assert torch.isfinite(y).all(), what
    frac = float((err > tight).double().mean())
    assert bool((err <= loose).all()), f"{what}: {int((err > loose).sum())} outside the loose bound"
    assert frac <= FLIP_FRAC, f"{what}: {frac:.3f} of the outputs outside fp32 slack + half an fp16 ulp"


def _rand16(g, shape, dev, scale=1.0):
    x = torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))
    return x.to(dev)


def _kind(common):
    from vtoonify_amd import _lib
    return _lib.lib().vt_conv2d_tile(ctypes.byref(K.make_conv_desc(**common))) // 100000000


@pytest.mark.parametrize("N,c,H,W,cout,k", [(2, 64, 11, 13, 1, 3), (1, 96, 9, 20, 3, 3), (2, 64, 7, 9, 3, 1),
                                            (1, 64, 258, 256, 1, 3)])   # (the last: 16 x 16 tiles, conv_thin16_kernel)
def test_fp16_thin_outputs_vs_float64(dev, N, c, H, W, cout, k):
    """conv_thin.hpp (kind 6, planar fp32 outputs) in fp16: plain (mask-like, ToRGB-like with the skip residual), and the Fusion
    gate's loader (in_absdiff + the AdaIN affine: cat[x, |x - other|] * scale + shift, rounded to fp16 in the loader)."""
    g = np.random.default_rng(5 + c + cout)
    pad = k // 2
    x16 = K.nchw_to_nhwc(_rand16(g, (N, c, H, W), dev), torch.float16)
    o16 = K.nchw_to_nhwc(_rand16(g, (N, c, H, W), dev), torch.float16)
    for gate in ((False, True) if cout == 1 else (False,)):   # (the loader form has a one-plane instance only)
        cin = 2 * c if gate else c
        w = _rand16(g, (cout, cin, k, k), dev, 1.0 / math.sqrt(cin * k * k))
        wp = K.pack_conv_weight(w, out_dtype=torch.float16)
        wq = wp.double().cpu().reshape(cout, k, k, cin).permute(0, 3, 1, 2)
        b = _rand16(g, (cout,), dev, 0.1)
        xq, oq = x16.double().cpu().permute(0, 3, 1, 2), o16.double().cpu().permute(0, 3, 1, 2)
        skip = _rand16(g, (N, cout, H, W), dev)
        out = skip.clone()
        common = dict(n=N, h=H, w=W, out_h=H, out_w=W, weight=wp, cout=cout, kh=k, kw=k, pad=pad, bias=b, out=out,
                      ld_out=0, out_layout=K.OUT_NCHW, out_dtype=K.VT_F32, dtype=K.VT_F16)
        if gate:
            sc = _rand16(g, (N, 2 * c), dev, 0.3) + 1.0
            sh = _rand16(g, (N, 2 * c), dev, 0.3)
            common.update(src0=x16, c0=c, ld0=c, src1=o16, c1=c, ld1=c, in_scale=sc, in_shift=sh, in_absdiff=1,
                          act=K.ACT_RELU_TANH)
            # the loader's arithmetic, in fp32, then its rounding to fp16
            cat = torch.cat([xq, (xq - oq).abs()], 1).float()
            a32 = cat * sc.cpu()[:, :, None, None] + sh.cpu()[:, :, None, None]
            a = _h(a32)
        else:
            common.update(src0=x16, c0=c, ld0=c, resid=out, beta=1.0)
            a = xq
        assert _kind(common) == 6
        K.conv2d(**common)
        y = out.double().cpu()
        conv = torch.nn.functional.conv2d(a, wq, b.double().cpu(), padding=pad)
        absc = torch.nn.functional.conv2d(a.abs(), wq.abs(), padding=pad)
        ref = torch.tanh(conv.clamp(min=0)) if gate else conv + skip.double().cpu()
        tight = 1e-5 * absc + 1e-6 * float(ref.abs().max())
        loose = tight + (2 * H16 * torch.nn.functional.conv2d(a.abs(), wq.abs(), padding=pad) if gate else 0.0)
        _check_internal(y, ref, tight, loose, f"thin gate={gate}")


def _upblur_case(dev, N, cin, H, W, cout, fir, env, want_kind, monkeypatch, hint=32):
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    g = np.random.default_rng(cin + cout + H)
    x16 = K.nchw_to_nhwc(_rand16(g, (N, cin, H, W), dev), torch.float16)
    wp = K.pack_conv_weight(_rand16(g, (cout, cin, 3, 3), dev, 1.0 / math.sqrt(cin * 9)), out_dtype=torch.float16)
    b = _rand16(g, (cout,), dev)
    firt = torch.from_numpy(fir.astype(np.float32)).to(dev)
    out = torch.full((N, 2 * H, 2 * W, cout + 8), float("nan"), dtype=torch.float16, device=dev)
    common = dict(src0=x16, c0=cin, ld0=cin, n=N, h=H, w=W, out_h=2 * H, out_w=2 * W, weight=wp, cout=cout, kh=3, kw=3,
                  bias=b, act=K.ACT_LRELU, gain=2 ** 0.5, out=out, ld_out=cout + 8, dtype=K.VT_F16, up_fir=firt,
                  tile_hint=hint)
    assert _kind(common) == want_kind, (env, _kind(common))
    K.conv2d(**common)
    assert torch.isnan(out[..., cout:].float()).all(), "slack channels written"
    y = out[..., :cout].double().cpu().permute(0, 3, 1, 2)
    xq = x16.double().cpu().permute(0, 3, 1, 2)
    wq = wp.double().cpu().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    z = _h(torch.nn.functional.conv_transpose2d(xq, wq.transpose(0, 1), stride=2))   # the z tile / rows: fp16
    kf = torch.from_numpy(fir.astype(np.float32)).double().flip(0, 1)[None, None].repeat(cout, 1, 1, 1)
    blur = lambda t: torch.nn.functional.conv2d(torch.nn.functional.pad(t, (1, 1, 1, 1)), kf, groups=cout)  # noqa: E731
    pre = blur(z) + b.double().cpu()[None, :, None, None]
    ref = torch.where(pre > 0, pre, 0.2 * pre) * math.sqrt(2)
    M = float(ref.abs().max())
    tight = 2e-5 * M + H16 * ref.abs()
    loose = tight + 2 * H16 * math.sqrt(2) * blur(z.abs())
    _check_internal(y, ref, tight, loose, f"upblur {env}")
    for k_ in env:
        monkeypatch.delenv(k_)


_K1 = np.array([1, 3, 3, 1], np.float64)
_FIR_STD = np.outer(_K1, _K1) / 64.0 * 4.0
_FIR_ODD = np.outer(_K1, np.array([0.9, 3.1, 2.7, 1.3])) / 64.0 * 4.0
_OFF = {"VT_UPBLUR_ROWS": "0", "VT_UPBLUR_FLAT": "0", "VT_UPBLUR_P8": "0", "VT_UPBLUR_TALL": "0"}
_UPBLUR = [   # (what, N, cin, H, W, cout, fir, env, kind, hint)
    ("tile 32ch", 1, 128, 9, 13, 40, _FIR_STD, _OFF, 5, 32),
    ("tile 16ch double-buffered", 1, 256, 7, 9, 40, _FIR_STD, dict(_OFF, VT_UPBLUR_DB="1"), 5, 16),
    ("tile P8 persistent", 1, 64, 15, 14, 32, _FIR_STD, dict(_OFF, VT_UPBLUR_P8="1"), 5, 32),
    ("tile tall", 1, 128, 23, 13, 40, _FIR_STD, dict(_OFF, VT_UPBLUR_TALL="1"), 5, 32),
    ("rows", 2, 64, 11, 19, 40, _FIR_STD, dict(_OFF, VT_UPBLUR_ROWS="1", VT_UPBLUR_WGS="3"), 9, 32),
    ("rows, FIR not fp16-exact", 1, 128, 9, 23, 32, _FIR_ODD, dict(_OFF, VT_UPBLUR_ROWS="1"), 9, 32),
    ("flat 16ch", 1, 256, 7, 11, 40, _FIR_STD, dict(_OFF, VT_UPBLUR_FLAT="1", VT_UPBLUR_FLAT_CN="16"), 10, 32),
    ("flat 32ch", 1, 256, 9, 7, 64, _FIR_STD, dict(_OFF, VT_UPBLUR_FLAT="1", VT_UPBLUR_FLAT_CN="32"), 10, 32),
]


@pytest.mark.parametrize("what,N,cin,H,W,cout,fir,env,kind,hint", _UPBLUR, ids=[u[0] for u in _UPBLUR])
def test_fp16_upblur_forms_vs_float64(dev, monkeypatch, what, N, cin, H, W, cout, fir, env, kind, hint):
    """conv_transpose2d(stride 2) + blur + bias + LeakyReLU in every up-sampling form (tile kernels with their double-buffered,
    P8 and tall variants; strip-marching rows; flat tiles) against float64 with the z intermediate rounded to fp16."""
    _upblur_case(dev, N, cin, H, W, cout, fir, env, kind, monkeypatch, hint)


_TORGB = [   # (cin, cout, H, W, hint, env, kind)
    (64, 128, 19, 37, P + 1000000 + 256128, {}, 1),
    (64, 128, 35, 37, P + 1000000 + 256128, {"VT_PATCHW_WGS": "2"}, 1),       # persistent patch tiles
    (64, 64, 21, 35, P + 1000000 + 256064, {"VT_PATCH_PIPE": "1"}, 1),        # pipelined
    (64, 64, 40, 37, P + 1000000 + 256064, {"VT_PATCHW_WGS": "2"}, 1),        # weights resident
    (64, 64, 9, 40, P + 1000000 + 128064, {}, 1),
    (32, 32, 17, 33, 0, {}, 3),                                                # persistent 32 -> 32
    (64, 128, 12, 20, 2 * P + 1000000 + 128128, {}, 2),                        # 1-D direct-to-LDS
]


@pytest.mark.parametrize("cin,cout,H,W,hint,env,kind", _TORGB)
def test_fp16_fused_torgb_vs_float64(dev, monkeypatch, cin, cout, H, W, hint, env, kind):
    """StyledConv + ToRGB in one launch in fp16: the activation (fp16 output bar) and the fp32 planes, whose operand is the
    activation as stored (fp16) times the fp16 ToRGB weights on the matrix cores; rgb_only on the persistent 32 -> 32 kernel."""
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    g = np.random.default_rng(cin + cout + H)
    N = 2
    x16 = K.nchw_to_nhwc(_rand16(g, (N, cin, H, W), dev), torch.float16)
    wp = K.pack_conv_weight(_rand16(g, (cout, cin, 3, 3), dev, 1.0 / math.sqrt(9 * cin)), out_dtype=torch.float16)
    b = _rand16(g, (cout,), dev)
    wrp = K.pack_conv_weight(_rand16(g, (3, cout, 1, 1), dev, 1.0 / math.sqrt(cout)), out_dtype=torch.float16)
    br = _rand16(g, (3,), dev)
    skip = _rand16(g, (N, 3, H, W), dev)
    xq = x16.double().cpu().permute(0, 3, 1, 2)
    wq = wp.double().cpu().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    wrq = wrp.double().cpu().reshape(3, cout)[:, :, None, None]
    pre = torch.nn.functional.conv2d(xq, wq, b.double().cpu(), padding=1)
    yref = torch.where(pre > 0, pre, 0.2 * pre) * math.sqrt(2)
    for rgb_only in ((0, 1) if kind == 3 else (0,)):
        out = torch.full((N, H, W, cout), 7.0, dtype=torch.float16, device=dev)
        rgb = skip.clone()
        common = dict(src0=x16, c0=cin, ld0=cin, n=N, h=H, w=W, out_h=H, out_w=W, weight=wp, cout=cout, kh=3, kw=3, pad=1,
                      bias=b, act=K.ACT_LRELU, gain=2 ** 0.5, out=out, ld_out=cout, dtype=K.VT_F16, tile_hint=hint,
                      rgb_weight=wrp, rgb_bias=br, rgb_resid=rgb, rgb_out=rgb, rgb_only=rgb_only)
        assert _kind(common) == kind
        K.conv2d(**common)
        y = out.double().cpu().permute(0, 3, 1, 2)
        if rgb_only:
            assert bool((y == 7.0).all()), "rgb_only stored the activation"
        else:
            assert bool(((y - yref).abs() <= 2e-5 * float(yref.abs().max()) + H16 * yref.abs()).all()), "activation"
        act = _h(yref)                       # the activation as stored: the ToRGB operand
        rref = torch.nn.functional.conv2d(act, wrq, br.double().cpu()) + skip.double().cpu()
        absr = torch.nn.functional.conv2d(act.abs(), wrq.abs())
        tight = 1e-5 * absr + 1e-6 * float(rref.abs().max())
        loose = tight + 2 * H16 * absr       # one fp16 ulp of every activation term
        _check_internal(rgb.double().cpu(), rref, tight, loose, f"ToRGB cin {cin} cout {cout} hint {hint} only {rgb_only}")


@pytest.mark.parametrize("split", [False, True])
def test_fp16_instnorm_records_vs_float64(dev, split):
    """vt_conv_desc.stats_part in fp16: the chunk records (x0, sum(x - x0), sum((x - x0)^2)) of the output AS STORED, from the
    split-K reduce pass (split) or the stand-alone statistics launch, against float64 on the stored fp16 values."""
    N, cin, H, W, cout = 2, 128, 16, 20, 64
    g = np.random.default_rng(9)
    x16 = K.nchw_to_nhwc(_rand16(g, (N, cin, H, W), dev), torch.float16)
    wp = K.pack_conv_weight(_rand16(g, (cout, cin, 3, 3), dev, 1.0 / math.sqrt(9 * cin)), out_dtype=torch.float16)
    hw = H * W
    cpx = min(max((hw + 255) // 256, 64), 4096)
    chunks = (hw + cpx - 1) // cpx
    recs = torch.full((N * chunks * cout * 3,), float("nan"), dtype=torch.float32, device=dev)
    out = torch.zeros((N, H, W, cout), dtype=torch.float16, device=dev)
    common = dict(src0=x16, c0=cin, ld0=cin, n=N, h=H, w=W, out_h=H, out_w=W, weight=wp, cout=cout, kh=3, kw=3, pad=1,
                  bias=_rand16(g, (cout,), dev), act=K.ACT_LRELU, gain=2 ** 0.5, out=out, ld_out=cout, dtype=K.VT_F16,
                  stats_part=recs, tile_hint=(P + 2000000 + 128064) if split else 0)
    if split:
        common["splitk_ws"] = torch.zeros(8 << 20, dtype=torch.float32, device=dev)
    K.conv2d(**common)
    y = out.double().cpu().reshape(N, hw, cout)
    r = recs.double().cpu().reshape(N, chunks, cout, 3)
    for ck in range(chunks):
        seg = y[:, ck * cpx:min(hw, (ck + 1) * cpx)]
        x0 = seg[:, :1]
        d = seg - x0
        assert torch.equal(r[:, ck, :, 0], x0[:, 0]), ck
        assert bool(((r[:, ck, :, 1] - d.sum(1)).abs() <= 1e-5 * d.abs().sum(1) + 1e-6).all()), ck
        assert bool(((r[:, ck, :, 2] - (d * d).sum(1)).abs() <= 1e-5 * (d * d).sum(1) + 1e-6).all()), ck


def test_fp16_adain_loader_vs_float64(dev):
    """The AdaIN affine in the conv loader (vt_conv_desc.in_scale / in_shift, register-staged kernel) in fp16: x * scale + shift
    in fp32, rounded to fp16, then the conv."""
    N, cin, H, W, cout = 2, 64, 9, 13, 64
    g = np.random.default_rng(21)
    x16 = K.nchw_to_nhwc(_rand16(g, (N, cin, H, W), dev), torch.float16)
    wp = K.pack_conv_weight(_rand16(g, (cout, cin, 3, 3), dev, 1.0 / math.sqrt(9 * cin)), out_dtype=torch.float16)
    sc = _rand16(g, (N, cin), dev, 0.3) + 1.0
    sh = _rand16(g, (N, cin), dev, 0.3)
    out = torch.full((N, H, W, cout + 8), float("nan"), dtype=torch.float16, device=dev)
    common = dict(src0=x16, c0=cin, ld0=cin, n=N, h=H, w=W, out_h=H, out_w=W, weight=wp, cout=cout, kh=3, kw=3, pad=1,
                  out=out, ld_out=cout + 8, dtype=K.VT_F16, in_scale=sc, in_shift=sh)
    assert _kind(common) == 0
    K.conv2d(**common)
    assert torch.isnan(out[..., cout:].float()).all()
    y = out[..., :cout].double().cpu().permute(0, 3, 1, 2)
    xq = x16.float().cpu().permute(0, 3, 1, 2)
    a = _h(xq * sc.cpu()[:, :, None, None] + sh.cpu()[:, :, None, None])
    wq = wp.double().cpu().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(a, wq, padding=1)
    absc = torch.nn.functional.conv2d(a.abs(), wq.abs(), padding=1)
    tight = 2e-5 * float(ref.abs().max()) + H16 * ref.abs()
    _check_internal(y, ref, tight, tight + 2 * H16 * absc, "AdaIN loader")
