"""VToonify with the reference's constructor, state_dict schema and forward signature
(model/vtoonify.py:130-286), executing on vtoonify_amd.engine.VToonifyEngine.

The module tree below only HOLDS parameters under the reference's names (399 state_dict
entries for backbone='dualstylegan', 229 for 'toonify') so that
`VToonify(backbone).load_state_dict(ckpt['g_ema'])` (style_transfer.py:62-64) works
unchanged; `generator` / `stylegan()` additionally carry their own forward (generator.py), which
VToonify.forward never calls.  With the parameters on a GPU all arithmetic happens in the HIP engine and nothing
falls back; with the parameters on the CPU (`style_transfer.py --cpu`, :32,55) the forward
pass is the reference's eager operator sequence over the CPU-tensor branch of the operator
surface (eager.py, op/native.py) -- the reference's own "CPU tensors -> native path" contract.
Initial values follow the reference initialisers (randn for StyleGAN2 weights, default
nn.Conv2d/nn.Linear init, identity-like T_s, x0.01 ModRes filters) but are not
bit-identical to it -- real use loads a checkpoint.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
from torch import nn

from . import _lib
from .eager import EagerVToonify
from .engine import VToonifyEngine
from .synth import fir_kernel_2d

_CH = {4: 512, 8: 512, 16: 512, 32: 512}


def _channels(mult: int):
    ch = dict(_CH)
    ch.update({64: 256 * mult, 128: 128 * mult, 256: 64 * mult, 512: 32 * mult, 1024: 16 * mult})
    return ch  # model/stylegan/model.py:422-432


class _P(nn.Module):
    """Bare parameter/buffer holder."""

    def __init__(self, params=None, buffers=None):
        super().__init__()
        for k, v in (params or {}).items():
            self.register_parameter(k, nn.Parameter(v))
        for k, v in (buffers or {}).items():
            self.register_buffer(k, v)


def _eq_linear(i, o, lr_mul=1.0, bias_init=0.0):
    return _P({"weight": torch.randn(o, i) / lr_mul, "bias": torch.full((o,), float(bias_init))})


def _mod_conv(cin, cout, k, style_dim, up):
    m = _P({"weight": torch.randn(1, cout, cin, k, k)})
    m.modulation = _eq_linear(style_dim, cin, bias_init=1.0)
    if up:
        m.blur = _P(buffers={"kernel": fir_kernel_2d(gain=4.0)})
    return m


def _styled_conv(cin, cout, style_dim, up):
    m = nn.Module()
    m.conv = _mod_conv(cin, cout, 3, style_dim, up)
    m.noise = _P({"weight": torch.zeros(1)})
    m.activate = _P({"bias": torch.zeros(cout)})
    return m


def _to_rgb(cin, style_dim, up=True):
    m = _P({"bias": torch.zeros(1, 3, 1, 1)})
    if up:
        m.upsample = _P(buffers={"kernel": fir_kernel_2d(gain=4.0)})
    m.conv = _mod_conv(cin, 3, 1, style_dim, False)
    return m


def _mapping(n, dim=512):
    seq = nn.Sequential(nn.Identity(), *[_eq_linear(dim, dim, lr_mul=0.01) for _ in range(n)])
    return seq  # index 0 = PixelNorm (parameter-free), 1..n = EqualLinear


class _StyleGAN2(nn.Module):
    """Parameter layout of Generator (model/stylegan/model.py:395-489)."""

    def __init__(self, size, style_dim, n_mlp, mult):
        super().__init__()
        self.size, self.style_dim = size, style_dim
        self.channels = _channels(mult)
        self.style = _mapping(n_mlp, style_dim)
        self.input = _P({"input": torch.randn(1, self.channels[4], 4, 4)})
        self.conv1 = _styled_conv(self.channels[4], self.channels[4], style_dim, False)
        self.to_rgb1 = _to_rgb(self.channels[4], style_dim, up=False)
        self.log_size = int(math.log2(size))
        self.num_layers = (self.log_size - 2) * 2 + 1
        self.n_latent = self.log_size * 2 - 2
        self.convs, self.to_rgbs = nn.ModuleList(), nn.ModuleList()
        self.upsamples = nn.ModuleList()
        self.noises = nn.Module()
        for i in range(self.num_layers):
            r = (i + 5) // 2
            self.noises.register_buffer(f"noise_{i}", torch.randn(1, 1, 2 ** r, 2 ** r))
        cin = self.channels[4]
        for i in range(3, self.log_size + 1):
            cout = self.channels[2 ** i]
            self.convs.append(_styled_conv(cin, cout, style_dim, True))
            self.convs.append(_styled_conv(cout, cout, style_dim, False))
            self.to_rgbs.append(_to_rgb(cout, style_dim))
            cin = cout


def _adain(c, style_dim):
    m = nn.Module()
    m.style = nn.Linear(style_dim, 2 * c)
    with torch.no_grad():
        m.style.bias[:c] = 1.0
        m.style.bias[c:] = 0.0
    return m


def _ada_res(c, style_dim=512):
    """AdaResBlock parameters (model/dualstylegan.py:24-36): conv/conv2 = [EqualConv2d, FusedLeakyReLU]."""
    m = nn.Module()
    for nm in ("conv", "conv2"):
        setattr(m, nm, nn.Sequential(_P({"weight": torch.randn(c, c, 3, 3) * 0.01}), _P({"bias": torch.zeros(c)})))
    m.norm, m.norm2 = _adain(c, style_dim), _adain(c, style_dim)
    return m


class _DualStyleGAN(nn.Module):
    """Parameter layout of DualStyleGAN (model/dualstylegan.py:47-82); generator.py's DualStyleGAN adds the forward."""
    _stylegan_cls = _StyleGAN2

    def __init__(self, size, style_dim, n_mlp, mult, res_index=6):
        super().__init__()
        self.style = _mapping(n_mlp - 6)
        self.generator = self._stylegan_cls(size, style_dim, n_mlp, mult)
        self.res = nn.ModuleList([_ada_res(self.generator.channels[4])])
        res_index = res_index // 2 * 2
        for i in range(3, self.generator.log_size + 1):
            c = self.generator.channels[2 ** i]
            for _ in range(2):
                if i < 3 + res_index // 2:
                    self.res.append(_ada_res(c))
                else:
                    self.res.append(self._identity_fc())
        self.res.append(self._identity_fc())
        g = self.generator
        self.size, self.style_dim, self.log_size = g.size, g.style_dim, g.log_size
        self.num_layers, self.n_latent, self.channels = g.num_layers, g.n_latent, g.channels

    @staticmethod
    def _identity_fc():
        m = _eq_linear(512, 512)
        with torch.no_grad():
            m.weight.copy_(torch.eye(512) * math.sqrt(512.0) + torch.randn(512, 512) * 0.01)
        return m


def _res_block(c):
    m = nn.Module()
    m.conv, m.conv2 = nn.Conv2d(c, c, 3, 1, 1), nn.Conv2d(c, c, 3, 1, 1)
    return m


def _fusion(c):
    """Fusion parameters (model/vtoonify.py:106-120)."""
    m = nn.Module()
    m.conv = nn.Conv2d(2 * c, c, 3, 1, 1)
    m.norm = _adain(2 * c, 128)
    m.conv2 = nn.Conv2d(2 * c, 1, 3, 1, 1)
    m.linear = nn.Sequential(nn.Linear(1, 64), nn.Identity(), nn.Linear(64, 128), nn.Identity())
    return m


class VToonify(nn.Module):
    def __init__(self, in_size=256, out_size=1024, img_channels=3, style_channels=512, num_mlps=8,
                 channel_multiplier=2, num_res_layers=6, backbone="dualstylegan",
                 compute_dtype: Optional[torch.dtype] = None, exact_fp32: Optional[bool] = None):
        """compute_dtype: the arithmetic the frame runs in.  None = the environment variable VTOONIFY_AMD_DTYPE
        ("fp32" | "fp32_exact" | "bf16" | "fp16"), default **fp32** -- the reference's own precision (it is fp32 end to end,
        model/stylegan/op/upfirdn2d_kernel.cu:311).  In fp32 every tensor, weight and non-conv kernel is fp32; the
        convolutions' products run on the bf16 matrix cores as three terms each (operands split into bf16 head + remainder
        in registers, fp32 accumulate: `VToonifyEngine(x3=True)`) -- 2-4e-5 of max|y| against the reference
        (the stated fp32 bar is 1e-4) at 1.5x the frame rate of the exact-fp32 matrix instructions, which remain one switch
        away: exact_fp32=True or VTOONIFY_AMD_DTYPE=fp32_exact (~5e-6, the bisection reference).  bf16 (PSNR >= 45 dB against
        the fp32 path) is an explicit choice: compute_dtype=torch.bfloat16 or VTOONIFY_AMD_DTYPE=bf16
        (INTEGRATION.md 0).  So is fp16 (compute_dtype=torch.float16 or VTOONIFY_AMD_DTYPE=fp16 / float16): the kernels, plans
        of bf16 at 0.98x its measured frame rate, with three more mantissa bits -- fp16 activations and weights, fp32 accumulation, statistics,
        style path and RGB skip path.  fp16 tops out at 65504: headroom on trained weights is unmeasured, and
        bf16 is the choice for a model that overflows."""
        super().__init__()
        env = os.environ.get("VTOONIFY_AMD_DTYPE", "fp32").lower()
        if (compute_dtype is None or exact_fp32 is None) and env not in ("fp32", "float32", "fp32x3", "fp32_exact", "bf16", "bfloat16",
                                                                         "fp16", "float16"):
            raise ValueError(f"VTOONIFY_AMD_DTYPE={env!r}: expected fp32 (= fp32x3), fp32_exact, bf16 or fp16")
        if compute_dtype is None:
            compute_dtype = (torch.bfloat16 if env.startswith("b") else torch.float16 if env in ("fp16", "float16")
                             else torch.float32)
        if exact_fp32 is None:
            exact_fp32 = env == "fp32_exact"
        self.exact_fp32 = bool(exact_fp32)
        # the arithmetic in force, by name: "fp32x3" (fp32 tensors, conv products as three bf16 MFMAs: the default), "fp32_exact"
        # (exact-fp32 matrix instructions, the bisection reference), "bf16" or "fp16" -- what a log line / bench.py should print
        self.precision = ({torch.bfloat16: "bf16", torch.float16: "fp16"}[compute_dtype]
                          if compute_dtype in (torch.bfloat16, torch.float16) else ("fp32_exact" if exact_fp32 else "fp32x3"))
        self.backbone = backbone
        self.in_size = in_size
        self.style_channels = style_channels
        self.compute_dtype = compute_dtype
        # the generators carry their own forward (generator.py: portrait stylisation, style-image and paired-data synthesis)
        # in this module's precision; VToonify.forward below never calls it
        from .generator import DualStyleGAN, Generator
        if backbone == "dualstylegan":
            self.generator = DualStyleGAN(out_size, style_channels, num_mlps, channel_multiplier)
        else:
            self.generator = Generator(out_size, style_channels, num_mlps, channel_multiplier)
        for m in (self.generator, self.stylegan()):
            m.compute_dtype, m.exact_fp32 = compute_dtype, self.exact_fp32
        ch = self.generator.channels
        enc_res = [2 ** i for i in range(int(math.log2(in_size)), 4, -1)]
        self.encoder = nn.ModuleList([nn.Sequential(
            nn.Conv2d(img_channels + 19, 32, 3, 1, 1), nn.Identity(),
            nn.Conv2d(32, ch[in_size], 3, 1, 1), nn.Identity())])
        for r in enc_res:
            c = ch[r]
            if r > 32:
                co = ch[r // 2]
                self.encoder.append(nn.Sequential(nn.Conv2d(c, co, 3, 2, 1), nn.Identity(),
                                                  nn.Conv2d(co, co, 3, 1, 1), nn.Identity()))
            else:
                self.encoder.append(nn.Sequential(*[_res_block(c) for _ in range(num_res_layers)]))
                self.encoder.append(nn.Conv2d(c, img_channels, 1, 1, 0))
        self.fusion_out, self.fusion_skip = nn.ModuleList(), nn.ModuleList()
        for r in enc_res[::-1]:
            c = ch[r]
            self.fusion_out.append(_fusion(c) if backbone == "dualstylegan" else nn.Conv2d(2 * c, c, 3, 1, 1))
            self.fusion_skip.append(nn.Conv2d(c + 3, 3, 3, 1, 1))
        if backbone == "dualstylegan":
            self.res = nn.ModuleList([_ada_res(ch[4])])
            for i in range(3, 6):
                self.res.append(_ada_res(ch[2 ** i]))
                self.res.append(_ada_res(ch[2 ** i]))
        self._engine: Optional[VToonifyEngine] = None
        self._engine_probe = None
        self.requires_grad_(False)
        # a weight load into ANY submodule (`model.generator.load_state_dict(...)`, the pattern of the
        # reference's training scripts and notebooks) drops the packed / pre-scaled weights of the engine
        for m in self.modules():
            m.register_load_state_dict_post_hook(self._on_weights_loaded)

    # -- engine lifetime: any device move / weight load invalidates the packed weights --
    def _on_weights_loaded(self, module, incompatible_keys):
        self._engine = None

    def invalidate(self):
        """Drop the packed weights (call after editing parameters in place, e.g. through `.data`)."""
        self._engine = None
        object.__setattr__(self, "_probe_epoch", self._probe_epoch + 1)

    def _apply(self, fn, *a, **k):
        self._engine = None
        object.__setattr__(self, "_probe_epoch", self._probe_epoch + 1)
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._engine = None
        object.__setattr__(self, "_probe_epoch", self._probe_epoch + 1)
        return super().load_state_dict(*a, **k)

    def _probe(self):
        """Fingerprint of EVERY parameter and buffer (storage address, in-place version counter): a `.to()`, a re-assignment
        of a submodule (`model.generator = ...`) and an in-place edit of any parameter (`p.mul_(...)`, `p.copy_(...)`) all
        change it and drop the packed weights.  Only edits through `.data` escape the version counters -- those need
        invalidate().  Walking the module tree costs ~2 ms (per call that was most of a 3.5 ms step), so the walk
        is cached as (owning dict, name, object) triples of every parameter, buffer and child module; every call checks that
        each dict still holds the SAME object under that name (~550 dict lookups, 0.1 ms) and reads the tensors' address /
        version.  A replacement at any depth -- `model.generator.convs[i] = ...`, `sub.load_state_dict(..., assign=True)`,
        `register_parameter` on a child, `child.to(...)` with parameters overwritten on conversion -- fails an identity check
        on the NEXT call and the tree is walked again (the 64-call window is gone)."""
        trip = getattr(self, "_probe_triples", None)
        fresh = trip is None or self._probe_epoch_seen != self._probe_epoch
        if not fresh:
            for d, n, o in trip:
                if d.get(n) is not o:
                    fresh = True
                    break
        if fresh:
            trip = []
            for m in self.modules():
                trip += [(m._modules, n, c) for n, c in m._modules.items()]
                trip += [(m._parameters, n, t) for n, t in m._parameters.items()]
                trip += [(m._buffers, n, t) for n, t in m._buffers.items()]
            object.__setattr__(self, "_probe_triples", trip)
            object.__setattr__(self, "_probe_tensors", [o for _, _, o in trip if isinstance(o, torch.Tensor)])
            object.__setattr__(self, "_probe_epoch_seen", self._probe_epoch)
        ts = self._probe_tensors
        h = len(trip)
        for t in ts:
            h = (h * 1000003 + t.data_ptr() * 31 + t._version) & 0xFFFFFFFFFFFFFFF
        return h

    _probe_epoch = 0

    def __setattr__(self, name, value):
        if isinstance(value, (torch.Tensor, torch.nn.Module)):
            object.__setattr__(self, "_probe_epoch", self._probe_epoch + 1)
        super().__setattr__(name, value)

    def engine(self) -> VToonifyEngine:
        if self._engine is not None and self._engine_probe != self._probe():
            self._engine = None
        if self._engine is None:
            dev = next(self.parameters()).device
            # style_gate: a video passes the same style rows on every call (as a new tensor: s_w.repeat(B,1,1),
            # style_transfer.py:176); the style path is then skipped on the device, bit-identical to recomputing it
            self._engine = VToonifyEngine(self.state_dict(), self.backbone, self.in_size,
                                          self.compute_dtype, dev,
                                          style_gate=os.environ.get("VT_STYLE_GATE", "1") != "0",
                                          x3=self.compute_dtype == torch.float32 and not self.exact_fp32)
            self._engine_probe = self._probe()
        return self._engine

    def forward(self, x, style, d_s=None, return_mask=False, return_feat=False):
        """Same contract as model/vtoonify.py:210-277: x (B,22,H,W), style W+ (B,18,512) or
        W (B,512); returns (B,3,4H,4W) un-clamped, or (image, masks) / (feat, skip).

        On a GPU the frame is one hipGraph replay (captured on the first call of a shape; one plan per
        calling stream), i.e. the path bench.py measures; whether the B style rows are identical is
        decided without a host sync for expand()ed / single-row styles and once per style tensor otherwise."""
        if self._on_cpu():
            with torch.no_grad():
                return EagerVToonify(self.state_dict(), self.backbone, self.in_size).forward(
                    x, style, d_s, return_mask=return_mask, return_feat=return_feat)
        return self.engine().forward(x, style, d_s, return_mask=return_mask, return_feat=return_feat)

    def _on_cpu(self) -> bool:
        """Parameters on the CPU and no test emulation bound: the reference's CPU path (`--cpu`)."""
        return next(self.parameters()).device.type == "cpu" and not _lib.emulation_injected()

    def stylegan(self):
        return self.generator.generator if self.backbone == "dualstylegan" else self.generator

    def zplus2wplus(self, zplus):
        if self._on_cpu():
            with torch.no_grad():
                return EagerVToonify(self.state_dict(), self.backbone, self.in_size).zplus2wplus(zplus)
        return self.engine().map_style(zplus)
