"""The Fusion block without its packed operand (include/vtoonify_amd_fusion.h): vt_conv2d_gate (the mask conv
that also writes f_E * m_E) and vt_conv2d_hdr (fusion_skip with the skip planes as a second source) against the launches
they replace, and VToonifyEngine(fused_gate=True) against fused_gate=False.  Host emulation (CPU suite) and, with -m gpu,
the MI355X.

Every comparison is on raw bits: the new forms do the operations of the old sequence in its order, so there is no tolerance
to derive.  Every output is allocated with slack and filled with NaN; ld padding and slack must keep the sentinel.

Kernel-level shapes: the 8 x 8-tile kernel at N = 2, 20 x 19 (3 x 3 ragged tiles) with one and three K steps of channels
(three: the four waves own unequal step counts) and ld of f_E larger than C; the 16 x 16-tile kernel (taken from 256 tiles per
image up) at N = 2, 250 x 241 (16 x 16 tiles, ragged right and bottom) with C = 32 and 64 (fp32: two and four K steps;
16-bit: one and two).

Engine-level shapes on the GPU: D batch 2 136 x 120 (loader form on the 8 x 8 tiles at the top level, two launches below),
D batch 1 256 x 256 (16 x 16 tiles), T batch 1 64 x 64 (no mask), eager launches and hipGraph replay.  The host emulation
runs a whole frame at ~7 ms per input pixel (136 x 120 x 2 would take minutes), so the CPU suite reaches the same plan
branches on 16 x 24 frames instead: VT_GATE_LOADER=2 puts the loader form (vt_conv2d_gate) on every level, the default
leaves every level of so small a frame on two launches (vt_fusion_pack without a header), T has no mask; the 16 x 16 tiles
are covered on the CPU by the kernel-level cases only.  fused_gate=True fuses a level with a mask only from 8192 pixels per
image up (where it measured faster), so the small frames -- and a second pass of the GPU cases -- use fused_gate="all".
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
DTYPES = (BF16, F16, F32)      # every type the gate loader form is compiled for
SLACK = 67
HDR = 64


def kstep(dtype):
    return 16 if dtype == F32 else 32


def nan_buf(n, dtype, dev):
    return torch.full((n + SLACK,), float("nan"), dtype=dtype, device=dev)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def all_nan(t):
    return bool(torch.isnan(t.detach().cpu().float()).all())


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def rnd(g, shape, dtype=F32, scale=1.0, shift=0.0):
    return torch.from_numpy((g.standard_normal(shape) * scale + shift).astype(np.float32)).to(dtype)


def strided(t, ld, dev):
    """(n, h, w, c) values in NaN-filled pixel rows of ld elements, + slack; returns the flat device buffer."""
    n, h, w, c = t.shape
    buf = torch.full((n * h * w * ld + SLACK,), float("nan"), dtype=t.dtype)
    buf[:n * h * w * ld].view(n, h, w, ld)[..., :c] = t
    return buf.to(dev)


# ------------------------------------------------------------------------------------------------ (a) vt_conv2d_gate
class Gate:
    """One random gate problem: f_G (ld = c), f_E (ld = c + 16), AdaIN scale / shift of the 2c channels, mask-conv weights."""

    def __init__(self, dev, dtype, n, h, w, c, seed):
        g = np.random.default_rng(seed)
        self.dev, self.dtype, self.n, self.h, self.w, self.c, self.lde = dev, dtype, n, h, w, c, c + 16
        self.fg = rnd(g, (n, h, w, c), dtype)
        self.fe = rnd(g, (n, h, w, c), dtype)
        self.sc = rnd(g, (n, 2 * c), F32, 0.5, 1.0)
        self.sh = rnd(g, (n, 2 * c), F32, 0.3)
        self.wt = rnd(g, (1, 9, 2 * c), dtype, 1.0 / np.sqrt(18 * c)).to(dev)     # packed layout (cout, taps, cin)
        self.bias = torch.tensor([0.05]).to(dev)

    def sub(self, i):
        """The problem of image i alone."""
        o = Gate.__new__(Gate)
        o.__dict__.update(self.__dict__)
        o.n, o.fg, o.fe, o.sc, o.sh = 1, self.fg[i:i + 1], self.fe[i:i + 1], self.sc[i:i + 1], self.sh[i:i + 1]
        return o

    def desc_kw(self, fg, fe, sc, sh, mask):
        return dict(src0=fg, c0=self.c, ld0=self.c, src1=fe, c1=self.c, ld1=self.lde, in_scale=sc, in_shift=sh, in_absdiff=1,
                    n=self.n, h=self.h, w=self.w, out_h=self.h, out_w=self.w, weight=self.wt, cout=1, kh=3, kw=3, pad=1,
                    bias=self.bias, act=_lib.ACT_RELU_TANH, out=mask, ld_out=0, out_layout=_lib.OUT_NCHW, out_dtype=K.VT_F32,
                    dtype=K.dt_code(self.dtype))

    def run(self, fused, ld_fem=None):
        """-> (mask (n, h, w) fp32, fem (n, h, w, ld_fem)) with the sentinel checks done."""
        dev, n, hw, c = self.dev, self.n, self.h * self.w, self.c
        ld_fem = ld_fem or c
        fg, fe = self.fg.contiguous().to(dev), strided(self.fe, self.lde, dev)
        sc, sh = self.sc.contiguous().to(dev), self.sh.contiguous().to(dev)
        mask = nan_buf(n * hw, F32, dev)
        fem = nan_buf(n * hw * ld_fem, self.dtype, dev)
        kw = self.desc_kw(fg, fe, sc, sh, mask)
        if fused:
            K.conv2d_gate(fem, ld_fem, **kw)
        else:
            assert ld_fem == c
            K.conv2d(**kw)
            K.fusion_pack(fem, c, fe, self.lde, mask, None, n, hw, c, K.dt_code(self.dtype), stream_of=fem)
        sync(dev)
        assert all_nan(mask[n * hw:]) and all_nan(fem[n * hw * ld_fem:]), "slack overwritten"
        rows = fem[:n * hw * ld_fem].view(n, self.h, self.w, ld_fem)
        assert all_nan(rows[..., c:]) or ld_fem == c, "ld padding of fem overwritten"
        assert not torch.isnan(mask[:n * hw]).any() and not torch.isnan(rows[..., :c].float()).any()
        return mask[:n * hw].view(n, self.h, self.w).clone(), rows[..., :c].clone()


GATE_SHAPES = [(20, 19, 1), (20, 19, 3), (250, 241, 0)]     # (h, w, K steps of channels; 0: C = 32 and 64 on the 16 x 16 tiles)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16", "fp32"))
@pytest.mark.parametrize("h,w,steps", GATE_SHAPES)
def test_gate_equals_conv_then_pack(dev, dtype, h, w, steps):
    """vt_conv2d_gate == vt_conv2d (same descriptor) + vt_fusion_pack(ld_out = C): mask plane and fem, bit for bit; fem rows
    with ld padding keep the sentinel; a frame inside the batch of two equals the frame alone."""
    for c in ((32, 64) if steps == 0 else (steps * kstep(dtype),)):
        p = Gate(dev, dtype, 2, h, w, c, 1000 + c + h)
        tile = _lib.lib().vt_conv2d_tile(C.byref(K.make_conv_desc(**p.desc_kw(
            p.fg.to(dev), strided(p.fe, p.lde, dev), p.sc.to(dev), p.sh.to(dev), nan_buf(2 * h * w, F32, dev)))))
        assert tile // 100000000 == 6 and (tile // 1000) % 1000 == (256 if steps == 0 else 64)   # thin kernel, 16x16 / 8x8 tiles
        m_old, f_old = p.run(False)
        m_new, f_new = p.run(True)
        assert same_bits(m_new, m_old), (dtype, c, "mask")
        assert same_bits(f_new, f_old), (dtype, c, "fem")
        assert float(m_old.max()) > 0 and float((m_old == 0).float().mean()) > 0.05      # relu(tanh(.)): both branches taken
        m_ld, f_ld = p.run(True, ld_fem=c + 24)                                            # ld_fem > C
        assert same_bits(m_ld, m_old) and same_bits(f_ld, f_old), (dtype, c, "ld_fem > C")
        if steps != 0 or c == 32:
            m1, f1 = p.sub(1).run(True)
            assert same_bits(m1, m_new[1:]) and same_bits(f1, f_new[1:]), (dtype, c, "image alone")


# ------------------------------------------------------------------------------------------------- (b) vt_conv2d_hdr
def _hdr_case(dev, dtype, n, h, w, c, seed, cout=3):
    g = np.random.default_rng(seed)
    hw, ld = h * w, c + 16
    fem = rnd(g, (n, h, w, c), dtype)
    skip = rnd(g, (n, 3, h, w), F32).to(dev)
    wt = rnd(g, (cout, 9, c + HDR), dtype, 1.0 / np.sqrt(9 * (c + 3))).to(dev)
    bias = rnd(g, (cout,), F32, 0.1).to(dev)

    def conv_kw(src, c0, ld0, nn, out):
        return dict(src0=src, c0=c0, ld0=ld0, n=nn, h=h, w=w, out_h=h, out_w=w, weight=wt, cout=cout, kh=3, kw=3, pad=1,
                    bias=bias, out=out, ld_out=0, out_layout=_lib.OUT_NCHW, out_dtype=K.VT_F32, dtype=K.dt_code(dtype))

    def old(i0, nn):
        f_e = strided(fem[i0:i0 + nn], ld, dev)
        packed = nan_buf(nn * hw * (c + HDR), dtype, dev)
        K.fusion_pack(packed, c + HDR, f_e, ld, None, skip[i0:i0 + nn].contiguous(), nn, hw, c, K.dt_code(dtype))
        out = nan_buf(nn * cout * hw, F32, dev)
        K.conv2d(**conv_kw(packed, c + HDR, c + HDR, nn, out))
        sync(dev)
        assert all_nan(out[nn * cout * hw:])
        return out[:nn * cout * hw].view(nn, cout, h, w).clone()

    def new(i0, nn):
        f_e = strided(fem[i0:i0 + nn], ld, dev)
        out = nan_buf(nn * cout * hw, F32, dev)
        K.conv2d_hdr(skip[i0:i0 + nn].contiguous(), 3, HDR, **conv_kw(f_e, c, ld, nn, out))
        sync(dev)
        assert all_nan(out[nn * cout * hw:]), "slack overwritten"
        assert not torch.isnan(out[:nn * cout * hw]).any()
        return out[:nn * cout * hw].view(nn, cout, h, w).clone()

    return old, new


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16", "fp32"))
@pytest.mark.parametrize("h,w,steps", GATE_SHAPES)
def test_hdr_equals_pack_then_conv(dev, dtype, h, w, steps):
    """vt_conv2d_hdr == vt_fusion_pack into a C + 64 tensor + vt_conv2d, bit for bit; a frame of the batch equals it alone."""
    for c in ((32, 64) if steps == 0 else (steps * kstep(dtype),)):
        old, new = _hdr_case(dev, dtype, 2, h, w, c, 2000 + c + h)
        y_old, y_new = old(0, 2), new(0, 2)
        assert same_bits(y_new, y_old), (dtype, c)
        assert float(y_old.abs().max()) > 0.1
        if steps != 0 or c == 32:
            assert same_bits(new(1, 1), y_new[1:]), (dtype, c, "image alone")
    if steps == 1:      # one output channel: the second weight fragment of the kernel form holds no channel
        old, new = _hdr_case(dev, dtype, 1, h, w, kstep(dtype), 7, cout=1)
        assert same_bits(new(0, 1), old(0, 1)), (dtype, "cout 1")


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(dev):
    """Descriptors that are not the gate / header form, hdr_c > hdr_pad and a hdr_pad off the K step: VT_ERR_UNSUPPORTED with a
    message, and no byte of the outputs written."""
    lib = _lib.lib()
    UNSUPPORTED = 2     # VT_ERR_UNSUPPORTED
    p = Gate(dev, BF16, 1, 12, 9, 32, 5)
    fg, fe = p.fg.contiguous().to(dev), strided(p.fe, p.lde, dev)
    sc, sh = p.sc.to(dev), p.sh.to(dev)
    mask, fem = nan_buf(12 * 9, F32, dev), nan_buf(12 * 9 * 32, BF16, dev)
    stream = K._stream(mask)

    def gate(**over):
        kw = p.desc_kw(fg, fe, sc, sh, mask)
        kw.update(over)
        d = K.make_conv_desc(**kw)
        return lib.vt_conv2d_gate(C.byref(d), C.c_void_p(fem.data_ptr()), 32, stream)

    w1 = rnd(np.random.default_rng(1), (2, 9, 64), BF16).to(dev)
    assert gate(in_absdiff=0, src1=None, c1=0, ld1=0, in_scale=None, in_shift=None) == UNSUPPORTED     # a plain thin conv
    assert b"vt_conv2d_gate" in lib.vt_last_error()
    assert gate(cout=2, weight=w1) == UNSUPPORTED                                                       # two output channels
    assert gate(kh=1, kw=1, pad=0) == UNSUPPORTED                                                       # 1 x 1
    assert gate(pad=2, out_h=14, out_w=11) == UNSUPPORTED
    assert gate(out_layout=_lib.OUT_NHWC, ld_out=8) == UNSUPPORTED                                      # not a thin-output conv
    skip = rnd(np.random.default_rng(2), (1, 3, 12, 9)).to(dev)
    wt = rnd(np.random.default_rng(3), (3, 9, 32 + HDR), BF16).to(dev)
    out = nan_buf(3 * 12 * 9, F32, dev)

    def hdr(hdr_c=3, hdr_pad=HDR, **over):
        kw = dict(src0=fg, c0=32, ld0=32, n=1, h=12, w=9, out_h=12, out_w=9, weight=wt, cout=3, kh=3, kw=3, pad=1, out=out,
                  ld_out=0, out_layout=_lib.OUT_NCHW, out_dtype=K.VT_F32, dtype=K.VT_BF16)
        kw.update(over)
        d = K.make_conv_desc(**kw)
        return lib.vt_conv2d_hdr(C.byref(d), C.c_void_p(skip.data_ptr()), hdr_c, hdr_pad, stream)

    assert hdr(hdr_c=65) == UNSUPPORTED and b"vt_conv2d_hdr" in lib.vt_last_error()                     # hdr_c > hdr_pad
    assert hdr(hdr_pad=48) == UNSUPPORTED                                                               # not a multiple of 32
    assert hdr(hdr_pad=0, hdr_c=0) == UNSUPPORTED
    assert hdr(kh=1, kw=1, pad=0) == UNSUPPORTED
    assert hdr(src1=fe, c1=32, ld1=p.lde) == UNSUPPORTED                                                # two sources
    assert hdr(cout=8, out_layout=_lib.OUT_NHWC, ld_out=8, out_dtype=K.VT_BF16) == UNSUPPORTED
    sync(dev)
    assert all_nan(mask) and all_nan(fem) and all_nan(out), "a refused call wrote its output"
    assert hdr() == 0 and gate() == 0                                                                   # (the forms themselves run)
    sync(dev)
    assert not torch.isnan(out[:3 * 12 * 9]).any() and not torch.isnan(mask[:12 * 9]).any()


# ------------------------------------------------------------------------------------------------------------ engine
BB = {"D": "dualstylegan", "T": "toonify"}


def _engine_run(dev, tag, b, h, w, fused, graph):
    """-> ([(frames, masks) eager (, replay)], kernel names of the synthesis ops)"""
    sd = {k: v.to(dev) for k, v in synth.synth_state_dict(load_keys(tag), 0).items()}
    x = synth.synth_frames(b, h, w, seed=3).to(dev)
    s = synth.synth_style(seed=17).to(dev)
    eng = VToonifyEngine(sd, BB[tag], 256, BF16, dev, fused_gate=fused)
    outs = []
    for use_graph in ((False, True) if graph else (False,)):
        r = eng.forward(x, s.repeat(b, 1, 1), 0.5 if tag == "D" else None, return_mask=True, use_graph=use_graph)
        outs.append(r if isinstance(r, tuple) else (r, []))
    return outs, [op[2].get("kernel", "") for op in eng._plans[next(iter(eng._plans))].gen_ops]


def _check_pair(old, new, tag, n_gate, n_pack, n_hdr):
    (old, k_old), (new, k_new) = old, new
    n_lvl = 4
    assert sum(k == "fusion_pack" for k in k_old) == n_lvl and not any("+" in k for k in k_old)      # today's launches
    assert sum(k.endswith("+hdr") for k in k_new) == n_hdr
    assert sum(k.endswith("+fem") for k in k_new) == n_gate and sum(k == "fusion_pack" for k in k_new) == n_pack
    for (y0, m0), (y1, m1) in zip(old, new):
        assert same_bits(y1, y0), "frames differ"
        assert len(m1) == len(m0) == (n_lvl if tag == "D" else 0)
        for a, b in zip(m0, m1):
            assert same_bits(b, a), "masks differ"
    if len(new) == 2:                                                                                  # eager == hipGraph replay
        assert same_bits(new[1][0], new[0][0]) and all(same_bits(a, b) for a, b in zip(new[0][1], new[1][1]))


@pytest.mark.parametrize("case", ("D-loader", "D-two-launch", "T"))
def test_engine_fused_gate_on_small_frames(case, monkeypatch):
    """CPU suite (host emulation): fused_gate="all" == fused_gate=False on one 16 x 24 frame -- the loader form on every level
    (VT_GATE_LOADER=2: vt_conv2d_gate, no pack), two launches on every level (the default at this size: vt_fusion_pack
    with ld_out = C) and the Toonify backbone (no mask: fusion reads f_E itself).  (fused_gate=True fuses no level with a
    mask below 8192 pixels: the launch counts of the GPU cases pin that rule.)"""
    from emu import build_emu
    _lib.use_library(build_emu.build())
    dev = torch.device("cpu")
    if case == "D-loader":
        monkeypatch.setenv("VT_GATE_LOADER", "2")
    tag = case[0]
    args = (dev, tag, 1, 16, 24 if tag == "D" else 16)
    old, new = _engine_run(*args, False, False), _engine_run(*args, "all", False)
    _check_pair(old, new, tag, n_gate=4 if case == "D-loader" else 0, n_pack=4 if case == "D-two-launch" else 0, n_hdr=4)


GPU_CASES = (   # tag, batch, h, w, {fused_gate: (vt_conv2d_gate launches, vt_fusion_pack launches, vt_conv2d_hdr launches)}
    ("D", 2, 136, 120, {True: (1, 3, 1), "all": (1, 3, 4)}),
    ("D", 1, 256, 256, {True: (2, 2, 2), "all": (3, 1, 4)}),
    ("T", 1, 64, 64, {True: (0, 0, 4)}),
)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,b,h,w,want", GPU_CASES, ids=("D-2x136x120", "D-1x256x256", "T-1x64x64"))
def test_engine_fused_gate_on_the_gpu(tag, b, h, w, want):
    """MI355X: fused_gate=True (and "all") == fused_gate=False, frames and masks, eager launches and hipGraph replay.
    D 2 x 136 x 120: the loader form on 8 x 8 tiles at the top level (16 320 pixels), two launches on the three below (< 4096
    pixels).  D 256 x 256: the 16 x 16 tiles at 256^2, 8 x 8 tiles at 128^2 and 64^2, two launches at 32^2; True fuses the two
    levels from 8192 pixels up, "all" every level.  T: no mask, every level fused."""
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    _lib.use_library(_lib.DEFAULT_LIB)
    dev = torch.device("cuda:0")
    old = _engine_run(dev, tag, b, h, w, False, True)
    for fused, (n_gate, n_pack, n_hdr) in want.items():
        new = _engine_run(dev, tag, b, h, w, fused, True)
        _check_pair(old, new, tag, n_gate, n_pack, n_hdr)
        if (h, w) == (256, 256):
            assert any("256x" in k and k.endswith("+fem") for k in new[1]) and any("256x" in k and k.endswith("+hdr") for k in new[1])


# ------------------------------------------------------------------------------------------------------------ header
def test_fusion_header_binding_and_export():
    """include/vtoonify_amd_fusion.h as tests/test_frame_scale.py treats the frames header: what it declares is what _lib binds
    (its own dict, not the list pinned to vtoonify_amd.h), the gfx950 library exports it, the main header includes it."""
    from vtoonify_amd import build
    src = open(os.path.join(REPO, "include", "vtoonify_amd_fusion.h")).read()
    declared = sorted(set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.FUSION_SYMBOLS) == ["vt_conv2d_gate", "vt_conv2d_hdr"]
    others = set(_lib.EXPORTED_SYMBOLS) | set(_lib.PREPASS_SYMBOLS) | set(_lib.FRAMES_SYMBOLS)
    assert not set(declared) & others
    assert '#include "vtoonify_amd_fusion.h"' in open(os.path.join(REPO, "include", "vtoonify_amd.h")).read()
    lib = C.CDLL(build.build(verbose=False))
    for name in declared:
        assert hasattr(lib, name), name
        # the declaration's parameter list against the bound signature, in order
        decl = re.search(r"int " + name + r"\(([^)]*)\)", src).group(1)
        kinds = [C.POINTER(_lib.ConvDesc) if "vt_conv_desc" in a else
                 C.c_void_p if ("*" in a or "vt_stream" in a) else C.c_int32 for a in decl.split(",")]
        res, args = _lib._FUSION_SIGS[name]
        assert res is C.c_int and args == kinds, name
        block = src[:src.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert block.rstrip().endswith("*/") and re.search(r"vtoonify\.py:\d+", block)
    # vt_conv_desc did not grow: the new forms take their extras as arguments
    assert C.sizeof(_lib.ConvDesc) == 352
