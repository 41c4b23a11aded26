"""Upsample(skip) inside the fused-ToRGB epilogue (include/vtoonify_amd_rgbup.h): vt_conv2d_rgbup against the two
launches it replaces -- vt_upfirdn2d (up 2, pad (2, 1)) into the hi-res planes, then vt_conv2d with rgb_resid = rgb_out = those
planes.  Nothing is compared through a tolerance: the epilogue repeats the up-sampling launch operation for operation, so
planes and activation are the SAME BITS, for the engine's FIR and for a random non-symmetric one (a flipped or transposed tap
order is invisible to [1, 3, 3, 1]).  The new path gets its hi-res planes pre-filled with NaN -- as rgb_out and as the
descriptor's rgb_resid -- so a single read of them would show in the result.

Shapes: 40 x 56 hi-res on the persistent 32 -> 32 kernel is 3 x 4 tiles of 16 x 16, ragged on the right and at the bottom, once
with one tile per workgroup and once with workgroups that walk several tiles (VT_C32_BLOCKS).  The weights-resident patch
form is chosen by N * tiles >= 2 * persistent workgroups: 2 x 250 x 262 (neither size a multiple of 16) is the smallest batch
of that rule on the 256 compute units of an MI355X; the same kernel on 2 x 40 x 38 with VT_PATCHW_WGS=2 (the library's test
hook) covers its ragged tiles, both wave groups and uneven tile ranges in the emulation as well.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_keys
from vtoonify_amd import _lib, kernels as K, synth
from vtoonify_amd.engine import VToonifyEngine

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SLACK = 67
UNSUPPORTED = 2     # VT_ERR_UNSUPPORTED
FIR_ENGINE = (np.outer([1, 3, 3, 1], [1, 3, 3, 1]) / 64.0 * 4.0).astype(np.float32)     # make_kernel([1, 3, 3, 1]) * up^2
FIR_RANDOM = np.random.default_rng(77).standard_normal((4, 4)).astype(np.float32)       # no symmetry of any kind


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def rnd(g, shape, dtype=F32, scale=1.0):
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32)).to(dtype)


def lo_planes(g, n, h, w):
    """fp32 planes of mixed magnitude (1e-6 .. 1e3) with +0 and -0 among them -- also on the border rows and columns, where
    they meet the zeros of the padding."""
    v = g.standard_normal((n, 3, h, w)) * 10.0 ** g.integers(-6, 4, (n, 3, h, w))
    z = g.random((n, 3, h, w))
    v = np.where(z < 0.08, 0.0, np.where(z < 0.16, -0.0, v)).astype(np.float32)
    v[:, :, 0, ::3], v[:, :, -1, 1::3], v[:, :, ::2, 0], v[:, :, 1::2, -1] = -0.0, 0.0, 0.0, -0.0
    return torch.from_numpy(v)


class Case:
    """One random StyledConv + ToRGB problem: cin -> cout at (n, hh, ww) hi-res, lo-res planes of (hh / 2, ww / 2)."""

    def __init__(self, dev, dtype, n, hh, ww, c, seed):
        g = np.random.default_rng(seed)
        self.dev, self.dtype, self.n, self.hh, self.ww, self.c = dev, dtype, n, hh, ww, c
        self.x = K.nchw_to_nhwc(rnd(g, (n, c, hh, ww)).to(dev), dtype)
        self.wt = K.pack_conv_weight(rnd(g, (c, c, 3, 3), scale=1.0 / np.sqrt(9 * c)).to(dev), out_dtype=dtype)
        self.bias = rnd(g, (c,)).to(dev)
        self.rgbw = K.pack_conv_weight(rnd(g, (3, c, 1, 1), scale=1.0 / np.sqrt(c)).to(dev), out_dtype=dtype)
        self.rgbb = rnd(g, (3,)).to(dev)
        self.lo = lo_planes(g, n, hh // 2, ww // 2).to(dev)

    def desc_kw(self, out, rgb, **over):
        kw = dict(src0=self.x, c0=self.c, ld0=self.c, n=self.n, h=self.hh, w=self.ww, out_h=self.hh, out_w=self.ww,
                  weight=self.wt, cout=self.c, kh=3, kw=3, pad=1, bias=self.bias, act=K.ACT_LRELU, gain=2 ** 0.5, out=out,
                  ld_out=self.c, dtype=K.dt_code(self.dtype), rgb_weight=self.rgbw, rgb_bias=self.rgbb, rgb_resid=rgb,
                  rgb_out=rgb)
        kw.update(over)
        return kw

    def bufs(self, rgb_fill):
        n, hh, ww, c, dev = self.n, self.hh, self.ww, self.c, self.dev
        out = torch.full((n * hh * ww * c + SLACK,), 7.0, dtype=self.dtype, device=dev)
        rgb = torch.full((n * 3 * hh * ww + SLACK,), rgb_fill, dtype=F32, device=dev)
        return out, rgb

    def run(self, fold, fir, **over):
        """-> (activation (n, hh, ww, c), planes (n, 3, hh, ww)), slack checked."""
        n, hh, ww, c, dev = self.n, self.hh, self.ww, self.c, self.dev
        out, rgb = self.bufs(float("nan") if fold else 0.0)
        if fold:
            K.conv2d_rgbup(self.lo, fir, **self.desc_kw(out, rgb, **over))
        else:
            up = K.upfirdn2d_planes(self.lo.view(n * 3, hh // 2, ww // 2), fir, 2, 2, 1, 1, 2, 1, 2, 1)
            assert up.shape == (n * 3, hh, ww)
            rgb[:n * 3 * hh * ww] = up.reshape(-1)
            K.conv2d(**self.desc_kw(out, rgb, **over))
        sync(dev)
        assert bool((out[n * hh * ww * c:] == 7.0).all()), "activation slack overwritten"
        tail = rgb[n * 3 * hh * ww:]
        assert bool(torch.isnan(tail).all() if fold else (tail == 0.0).all()), "plane slack overwritten"
        planes = rgb[:n * 3 * hh * ww].view(n, 3, hh, ww).clone()
        assert not torch.isnan(planes).any()
        return out[:n * hh * ww * c].view(n, hh, ww, c).clone(), planes


def _kind(p, **over):
    out, rgb = p.bufs(0.0)
    return _lib.lib().vt_conv2d_tile(C.byref(K.make_conv_desc(**p.desc_kw(out, rgb, **over))))


def _pair(p, fir, what, **over):
    a_old, r_old = p.run(False, fir, **over)
    a_new, r_new = p.run(True, fir, **over)
    assert same_bits(r_new, r_old), (what, "planes")
    assert same_bits(a_new, a_old), (what, "activation")
    return a_new, r_new


# ----------------------------------------------------------------------------------------------- (1) persistent 32 -> 32
@pytest.mark.parametrize("fir", (FIR_ENGINE, FIR_RANDOM), ids=("fir1331", "firrandom"))
@pytest.mark.parametrize("dtype", (BF16, F16), ids=("bf16", "fp16"))
def test_c32_fold_equals_upsample_then_conv(dev, monkeypatch, dtype, fir):
    """conv3x3_c32_kernel: N = 2, 32 -> 32, 40 x 56 (3 x 4 ragged tiles), LeakyReLU * sqrt(2), ToRGB with bias, with the
    activation stored and with rgb_only; one tile per workgroup and five workgroups walking the 24 tiles."""
    p = Case(dev, dtype, 2, 40, 56, 32, 11)
    fir = torch.from_numpy(fir).to(dev)
    assert _kind(p) // 100000000 == 3
    for blocks in (None, "5"):
        if blocks:
            monkeypatch.setenv("VT_C32_BLOCKS", blocks)
        for rgb_only in (0, 1):
            act, planes = _pair(p, fir, (dtype, blocks, rgb_only), rgb_only=rgb_only)
            if rgb_only:
                assert bool((act == 7.0).all()), "rgb_only stored the activation"
            else:
                assert float(act.float().abs().max()) > 0 and bool((act.float() < 0).any())      # both LeakyReLU branches
    # the up-sampled skip really is in the planes: other lo-res planes, other result
    q = Case(dev, dtype, 2, 40, 56, 32, 11)
    q.lo = q.lo * 2.0
    assert not same_bits(q.run(True, fir)[1], planes)


# ------------------------------------------------------------------------------------------- (2) weights-resident patch form
def _resident_case(dev, dtype, n, hh, ww, **over):
    p = Case(dev, dtype, n, hh, ww, 64, 23)
    tile = _kind(p, **over)
    assert tile // 100000000 == 1 and tile % 1000000 == 256064 and (tile // 1000000) % 100 <= 1
    for fir in (FIR_ENGINE, FIR_RANDOM):
        _pair(p, torch.from_numpy(fir).to(dev), (dtype, n, hh, ww), **over)


@pytest.mark.parametrize("dtype", (BF16, F16), ids=("bf16", "fp16"))
def test_resident_fold_equals_upsample_then_conv(dev, monkeypatch, dtype):
    """conv_patchw_kernel, 64 -> 64, on two persistent workgroups (VT_PATCHW_WGS): 2 x 40 x 38 is 18 ragged tiles, nine per
    workgroup, five and four per wave group; the tile hint asks for the 256 x 64 patch tiles that the plan gives images of
    the 512^2 level by itself.  vt_conv2d_rgbup runs such a plan on the resident form or refuses, so a pass also proves which
    kernel ran."""
    monkeypatch.setenv("VT_PATCHW_WGS", "2")
    _resident_case(dev, dtype, 2, 40, 38, tile_hint=100000000 + 256064)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", (BF16, F16), ids=("bf16", "fp16"))
def test_resident_fold_at_the_launch_rules_smallest_batch(dtype):
    """The same without the hook, where the library's own rule (N * tiles >= 2 * compute units) first chooses the resident
    form on an MI355X: N = 2 at 250 x 262, 544 tiles on 256 workgroups, neither size a multiple of 16."""
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    _lib.use_library(_lib.DEFAULT_LIB)
    _resident_case(torch.device("cuda:0"), dtype, 2, 250, 262)


# --------------------------------------------------------------------------------------------------------- (3) refusals
def test_refusals_launch_nothing(dev):
    """No fused ToRGB, an odd hi-res size, a descriptor that resolves to another kernel form (the pipelined 256 x 128 patch
    tiles; a 64 -> 64 conv too small for the resident form): VT_ERR_UNSUPPORTED with a message, outputs untouched."""
    lib = _lib.lib()
    fir = torch.from_numpy(FIR_ENGINE).to(dev)

    def call(p, out, rgb, **over):
        d = K.make_conv_desc(**p.desc_kw(out, rgb, **over))
        return lib.vt_conv2d_rgbup(C.byref(d), C.c_void_p(p.lo.data_ptr()), C.c_void_p(fir.data_ptr()), K._stream(rgb))

    touched = []
    p = Case(dev, BF16, 1, 24, 20, 32, 3)
    out, rgb = p.bufs(float("nan"))
    assert call(p, out, rgb, rgb_weight=None, rgb_bias=None, rgb_resid=None, rgb_out=None) == UNSUPPORTED      # no fused ToRGB
    assert b"vt_conv2d_rgbup" in lib.vt_last_error()
    touched.append((out, rgb))
    o = Case(dev, BF16, 1, 23, 20, 32, 4)                                                                       # odd height
    o.lo = lo_planes(np.random.default_rng(1), 1, 12, 10).to(dev)
    out, rgb = o.bufs(float("nan"))
    assert call(o, out, rgb) == UNSUPPORTED and b"vt_conv2d_rgbup" in lib.vt_last_error()
    touched.append((out, rgb))
    o = Case(dev, BF16, 1, 24, 21, 32, 5)                                                                       # odd width
    o.lo = lo_planes(np.random.default_rng(2), 1, 12, 11).to(dev)
    out, rgb = o.bufs(float("nan"))
    assert call(o, out, rgb) == UNSUPPORTED
    touched.append((out, rgb))
    s = Case(dev, BF16, 1, 24, 20, 64, 6)                              # 64 -> 64, 4 tiles: a patch plan, not the resident form
    assert _kind(s) // 100000000 not in (3,)
    out, rgb = s.bufs(float("nan"))
    assert call(s, out, rgb) == UNSUPPORTED and b"vt_conv2d_rgbup" in lib.vt_last_error()
    touched.append((out, rgb))
    sync(dev)
    for out, rgb in touched:
        assert bool((out == 7.0).all()) and bool(torch.isnan(rgb).all()), "a refused call wrote its output"
    out, rgb = p.bufs(float("nan"))
    assert call(p, out, rgb) == 0                                                                              # (the form itself runs)
    sync(dev)
    assert not torch.isnan(rgb[:3 * 24 * 20]).any()


# ------------------------------------------------------------------------------------------------------------ (4) engine
def _engine_run(dev, h, w, fold):
    sd = {k: v.to(dev) for k, v in synth.synth_state_dict(load_keys("D"), 0).items()}
    x = synth.synth_frames(2, h, w, seed=3).to(dev)
    s = synth.synth_style(seed=17).to(dev)
    eng = VToonifyEngine(sd, "dualstylegan", 256, BF16, dev, fold_rgb_up=fold)
    y = eng.forward(x, s.repeat(2, 1, 1), 0.5, use_graph=False).clone()
    return y, [op[2].get("kernel", "") for op in eng._plans[next(iter(eng._plans))].gen_ops]


def _engine_on_against_off(dev, h, w):
    y_off, k_off = _engine_run(dev, h, w, False)
    y_on, k_on = _engine_run(dev, h, w, True)
    assert same_bits(y_on, y_off)
    ups = [i for i, k in enumerate(k_off) if k.startswith("upfirdn2d_tile")]
    folded = [k for k in k_on if k.endswith(".up")]
    assert not any(k.endswith(".up") for k in k_off) and len(ups) == 5
    # only the last level (32 -> 32 on the persistent kernel) runs a form that folds at this size ...
    assert len(folded) == 1 and folded[0].startswith("conv3x3_c32_kernel")
    # ... so the op list is today's without the last up-sampling launch, in the same order, every other level untouched
    rest_off = list(k_off)
    del rest_off[ups[-1]]
    assert [k[:-3] if k.endswith(".up") else k for k in k_on] == rest_off


def test_engine_fold_on_against_off_small_frames():
    """CPU suite (host emulation): D backbone, bf16, 2 x 16 x 16 frames (the engine tests' size class in the emulation, where
    2 x 64 x 64 takes half a minute): fold_rgb_up=True against False, the same frames bit for bit; the op list is shorter by
    exactly the folded launch."""
    from emu import build_emu
    _lib.use_library(build_emu.build())
    _engine_on_against_off(torch.device("cpu"), 16, 16)


@pytest.mark.gpu
def test_engine_fold_on_against_off_on_the_gpu():
    """MI355X: D backbone, B = 2, 64 x 64 frames, bf16.  At this size only the 32 -> 32 form qualifies (the 64 -> 64 level has
    2 x 64 tiles, below two per persistent workgroup): the rule falls back cleanly at every other level."""
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    _lib.use_library(_lib.DEFAULT_LIB)
    _engine_on_against_off(torch.device("cuda:0"), 64, 64)


# ------------------------------------------------------------------------------------------------------------ header
def test_rgbup_header_binding_and_export():
    """include/vtoonify_amd_rgbup.h as the other additive headers are treated: what it declares is what _lib binds (its own
    dict), the gfx950 library exports it, the main header includes it, vt_conv_desc did not grow."""
    from vtoonify_amd import build
    src = open(os.path.join(REPO, "include", "vtoonify_amd_rgbup.h")).read()
    declared = sorted(set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.RGBUP_SYMBOLS) == ["vt_conv2d_rgbup"]
    others = set(_lib.EXPORTED_SYMBOLS) | set(_lib.PREPASS_SYMBOLS) | set(_lib.FRAMES_SYMBOLS) | set(_lib.FUSION_SYMBOLS)
    assert not set(declared) & others
    assert '#include "vtoonify_amd_rgbup.h"' in open(os.path.join(REPO, "include", "vtoonify_amd.h")).read()
    lib = C.CDLL(build.build(verbose=False))
    for name in declared:
        assert hasattr(lib, name), name
        decl = re.search(r"int " + name + r"\(([^)]*)\)", src).group(1)
        kinds = [C.POINTER(_lib.ConvDesc) if "vt_conv_desc" in a else
                 C.c_void_p if ("*" in a or "vt_stream" in a) else C.c_int32 for a in decl.split(",")]
        res, args = _lib._RGBUP_SIGS[name]
        assert res is C.c_int and args == kinds, name
    assert C.sizeof(_lib.ConvDesc) == 352 and _lib.ABI_VERSION == 5
