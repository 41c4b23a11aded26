"""The kernel layer of the StyleGAN2 / DualStyleGAN generator forward (include/vtoonify_amd_generator.h, csrc/generator_ops.hip,
DESIGN.md 4.10): torch<->C-ABI adapters of its four entry points, and the definition of a forward call's random noise.

This module holds the pieces that model/stylegan/model.py:395-590 and model/dualstylegan.py:47-200 need beyond what the
VToonify plans already launch -- NoiseInjection with real noise, the tail of StyledConv.forward, truncation and the path mix.
`GeneratorEngine` strings them together with the existing conv / style / norm kernels into a launch plan per (batch, branch
set); `Generator` and `DualStyleGAN` are the reference's modules (constructor, state_dict schema, forward signature) on top
of it, and what `VToonify.stylegan()` / `VToonify.generator` are instances of.  A module whose parameters live on the CPU
runs the plain torch formulas (`EagerGenerator`, over the operator surface like eager.py), never the engine.

Random noise.  `draw_noise` is how a `randomize_noise=True` call gets its maps: ONE 64-bit key per call from torch's default
CPU generator (so `torch.manual_seed` reproduces a call), layer i's map = stream id i of that key, element index =
sample * H * W + pixel.  The values are statistically N(0,1); they are NOT the bits `torch.Tensor.normal_` would give for the
same seed (the reference draws `x.new_empty(B,1,H,W).normal_()` per layer on the GPU).  The key is drawn on the host, the maps
are written asynchronously on the current stream: nothing waits for the device.
"""
from __future__ import annotations

import ctypes as C
import math
import random
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import ACT_LRELU, ACT_NONE, OUT_NCHW
from .kernels import _dev_ok, _p, _stream, dt_code

SQRT2 = math.sqrt(2.0)


def philox_u32(blocks: int, ctr_lo: int, ctr_hi: int, key: int, device) -> torch.Tensor:
    """(blocks, 4) int32 tensor holding the uint32 words of Philox4x32-10 blocks (ctr_lo + i, ctr_hi) under `key`."""
    out = torch.empty((blocks, 4), dtype=torch.int32, device=device)
    _dev_ok(out)
    _lib.check(_lib.lib().vt_philox_u32(_p(out), blocks, ctr_lo, ctr_hi, key, _stream(out)), "vt_philox_u32")
    return out


def randn_into(out: torch.Tensor, key: int, stream_id: int, offset: int = 0) -> torch.Tensor:
    """Fill the contiguous fp32 tensor `out` with elements [offset, offset + numel) of the normal sequence (key, stream_id)."""
    _dev_ok(out)
    if out.dtype != torch.float32:
        raise _lib.VtError("randn: the output is fp32")
    _lib.check(_lib.lib().vt_randn(_p(out), out.numel(), offset, key, stream_id, _stream(out)), "vt_randn")
    return out


def randn(n: int, key: int, stream_id: int, device, offset: int = 0) -> torch.Tensor:
    return randn_into(torch.empty((n,), dtype=torch.float32, device=device), key, stream_id, offset)


def draw_key() -> int:
    """The 64-bit key of one forward call, from torch's default CPU generator (two 32-bit draws, low word first)."""
    lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
    return (hi << 32) | lo


def noise_sizes(size: int):
    """(H, W) of noises.noise_0 .. noise_{2 log2(size) - 3} (model/stylegan/model.py:454-460)."""
    log_size = int(math.log2(size))
    return [(2 ** ((i + 5) // 2),) * 2 for i in range((log_size - 2) * 2 + 1)]


def draw_noise(batch: int, size: int, device, key: int | None = None):
    """The noise list of one `randomize_noise=True` call on a generator of output `size`: map i is (batch,1,H_i,W_i) fp32,
    stream id i of `key` (default: `draw_key()`, which advances torch's default CPU generator by exactly one call's worth)."""
    if key is None:
        key = draw_key()
    return [randn(batch * h * w, key, i, device).view(batch, 1, h, w) for i, (h, w) in enumerate(noise_sizes(size))]


def noise_bias_act(x: torch.Tensor, noise: torch.Tensor, weight: torch.Tensor, bias, c: int | None = None, out=None):
    """lrelu(x + weight * noise + bias, 0.2) * sqrt(2) on an NHWC tensor x (B,H,W,ld) or (B,HW,ld) whose first `c` channels
    are data (default: all); noise (1 or B,1,H,W) fp32; weight a one-element fp32 tensor on the device; bias (c) fp32 or None.
    `out` defaults to a new tensor of x's shape; pass x itself for in-place use."""
    if out is None:
        out = torch.empty_like(x)
    _dev_ok(x, out, noise, weight, bias)
    if noise.dtype != torch.float32 or weight.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise _lib.VtError("noise_bias_act: noise, weight and bias are fp32")
    if out.dtype != x.dtype or out.shape != x.shape:
        raise _lib.VtError("noise_bias_act: out must have x's shape and dtype")
    b, ld = x.shape[0], x.shape[-1]
    hw = x.numel() // (b * ld)
    c = ld if c is None else c
    nb = noise.shape[0]
    if noise.numel() != nb * hw or (bias is not None and bias.numel() != c):
        raise _lib.VtError(f"noise_bias_act: noise {tuple(noise.shape)} / bias do not match x {tuple(x.shape)}")
    _lib.check(_lib.lib().vt_noise_bias_act(_p(out), ld, _p(x), ld, _p(noise), nb, _p(weight), _p(bias), b, hw, c,
                                            dt_code(x.dtype), _stream(x)), "vt_noise_bias_act")
    return out


def lerp_rows(a: torch.Tensor, b: torch.Tensor, f: torch.Tensor, out=None):
    """out[r] = f_r * b[r] + (1 - f_r) * a[r] on fp32 rows; a or b of one row broadcast; f one factor or one per row, on the
    device.  Truncation: a = truncation_latent, b = style, f = psi.  Path mix: a = w, b = T(e), f = interp_weight."""
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    _dev_ok(a2, b2, f)
    if not (a.dtype == b.dtype == f.dtype == torch.float32):
        raise _lib.VtError("lerp_rows: fp32 only")
    dim = a2.shape[1]
    rows = max(a2.shape[0], b2.shape[0])
    if b2.shape[1] != dim or a2.shape[0] not in (1, rows) or b2.shape[0] not in (1, rows) or f.numel() not in (1, rows):
        raise _lib.VtError(f"lerp_rows: shapes {tuple(a.shape)}, {tuple(b.shape)}, {tuple(f.shape)} do not match")
    if out is None:
        big = a if a2.shape[0] == rows else b
        out = torch.empty(big.shape, dtype=torch.float32, device=a.device)
    _dev_ok(out)
    ld_a = 0 if a2.shape[0] == 1 and rows > 1 else dim
    ld_b = 0 if b2.shape[0] == 1 and rows > 1 else dim
    _lib.check(_lib.lib().vt_lerp_rows(_p(out), dim, _p(a2), ld_a, _p(b2), ld_b, _p(f), 0 if f.numel() == 1 else 1, rows, dim,
                                       _stream(out)), "vt_lerp_rows")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# The same sequence on the host, for modules whose parameters live on the CPU (numpy; float64 inside, rounded to fp32:
# equal to the kernel's values to a few fp32 ulps, not to the bit)
def _philox_host(ctr_lo: np.ndarray, ctr_hi: int, key: int) -> np.ndarray:
    m32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    c0, c1 = ctr_lo & m32, ctr_lo >> sh
    c2 = np.full_like(ctr_lo, ctr_hi & 0xFFFFFFFF)
    c3 = np.full_like(ctr_lo, ctr_hi >> 32)
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m32, (p0 >> sh) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], axis=1)


def _randn_host(n: int, key: int, stream_id: int, offset: int = 0) -> torch.Tensor:
    j0, j1 = offset // 4, (offset + n - 1) // 4
    w = _philox_host(np.arange(j0, j1 + 1, dtype=np.uint64), stream_id, key)
    z = np.empty((w.shape[0], 4))
    two_pi = float(np.float32(2.0 * math.pi))
    for p in (0, 1):
        u = ((w[:, 2 * p] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        v = (w[:, 2 * p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u))
        z[:, 2 * p], z[:, 2 * p + 1] = r * np.cos(two_pi * v), r * np.sin(two_pi * v)
    return torch.from_numpy(z.reshape(-1)[offset - 4 * j0: offset - 4 * j0 + n].astype(np.float32))


def _host_device(device) -> bool:
    """A CPU device of a user (not the tests' emulation of the GPU library): the plain torch / numpy formulas."""
    return torch.device(device).type == "cpu" and not _lib.emulation_injected()


# ----------------------------------------------------------------------------------------------------------------------
# Host decisions shared by both executors, exactly the reference's (model.py:516-565, dualstylegan.py:102-145)
def _assemble_latent(styles, n_latent, inject_index, truncation, truncation_latent, input_is_latent, map_fn, trunc_fn):
    styles = list(styles)
    if not input_is_latent:
        styles = [map_fn(s.reshape(-1, s.shape[-1])).reshape(s.shape) for s in styles]
    if truncation < 1:
        styles = [trunc_fn(s, truncation_latent, truncation) for s in styles]
    if len(styles) < 2:
        return styles[0].unsqueeze(1).repeat(1, n_latent, 1) if styles[0].ndim < 3 else styles[0]
    if inject_index is None:
        inject_index = random.randint(1, n_latent - 1)
    if styles[0].ndim < 3:
        return torch.cat([styles[0].unsqueeze(1).repeat(1, inject_index, 1),
                          styles[1].unsqueeze(1).repeat(1, n_latent - inject_index, 1)], 1)
    return torch.cat([styles[0][:, 0:inject_index], styles[1][:, inject_index:]], 1)


def _check_styles(styles, input_is_latent, z_plus_latent):
    for s in styles:
        if not input_is_latent and s.ndim == 3 and not z_plus_latent:
            raise ValueError("z codes of shape (B, n_latent, dim) need z_plus_latent=True")


class _Branches:
    """Which layers of DualStyleGAN.forward take the extrinsic path (dualstylegan.py:158-183), decided on the host."""

    def __init__(self, n_latent, res_index, use_res, fuse_index, interp_weights):
        self.iw = [float(v) for v in interp_weights]
        self.modres = []      # ModRes block after latent row i
        self.mixed = []       # latent row i = iw * T_s(e_i) + (1 - iw) * w_i
        if not use_res:
            return
        if len(self.iw) < n_latent:
            raise ValueError(f"interp_weights needs {n_latent} entries")
        if fuse_index > 0 and self.iw[0] != 0:
            self.modres.append(0)
        for i in range(1, n_latent - 1, 2):
            for j in (i, i + 1):
                if fuse_index >= j and i > res_index:
                    self.mixed.append(j)
                if fuse_index >= j and i <= res_index and self.iw[j] != 0:
                    self.modres.append(j)
            if fuse_index >= i + 2 and i >= res_index - 1:
                self.mixed.append(i + 2)
        self.mixed = sorted(set(self.mixed))   # (ToRGB of one level and conv1 of the next read the same row, by the same rule)


# ----------------------------------------------------------------------------------------------------------------------
class EagerGenerator:
    """Generator.forward / DualStyleGAN.forward as the reference's operator sequence in plain torch over a VToonify-style
    state_dict (`generator.generator.*`, `generator.res.*`, `generator.style.*`; `generator.*` for a lone Generator): the
    executor of modules on the CPU."""

    def __init__(self, sd: Dict[str, torch.Tensor], dual: bool, size: int, res_index: int = 6):
        from .eager import EagerVToonify
        self.e = EagerVToonify(sd, "dualstylegan" if dual else "toonify")
        self.sd, self.g, self.dual, self.size = sd, self.e.g, dual, size
        self.log_size = int(math.log2(size))
        self.n_latent, self.num_layers = 2 * self.log_size - 2, 2 * (self.log_size - 2) + 1
        self.res_index = res_index // 2 * 2

    def _styled(self, x, style, name, up, noise):
        from .op import fused_leaky_relu
        y = self.e._modulated(x, style, name + "conv.", 3, True, up)
        return fused_leaky_relu(y + self.sd[name + "noise.weight"] * noise, self.sd[name + "activate.bias"])

    def _ada_res(self, x, s, w, i):
        if w == 0:
            return x
        name = f"generator.res.{i}."
        y = self.e._conv_layer(self.e._adain(x, s, name + "norm."), name + "conv.", 1)
        y = self.e._conv_layer(self.e._adain(y, s, name + "norm2."), name + "conv2.", 1)
        return y * w + x

    def map_style(self, z):
        return self.e._mapping(self.g + "style.", z)

    def noise_list(self, batch, noise, randomize_noise):
        if noise is not None:
            return list(noise)
        if randomize_noise:
            key = draw_key()
            return [_randn_host(batch * h * w, key, i).view(batch, 1, h, w) for i, (h, w) in enumerate(noise_sizes(self.size))]
        return [self.sd[f"{self.g}noises.noise_{i}"] for i in range(self.num_layers)]

    def forward(self, styles, exstyles=None, return_latents=False, return_feat=False, inject_index=None, truncation=1,
                truncation_latent=None, input_is_latent=False, noise=None, randomize_noise=True, z_plus_latent=False,
                use_res=True, fuse_index=18, interp_weights=(1,) * 18, return_feature_ind=999):
        sd, g = self.sd, self.g
        _check_styles(styles, input_is_latent, z_plus_latent)
        latent = _assemble_latent(styles, self.n_latent, inject_index, truncation, truncation_latent, input_is_latent,
                                  self.map_style, lambda s, t, psi: t + psi * (s - t))
        b, latent0 = latent.shape[0], latent
        noise = self.noise_list(b, noise, randomize_noise)
        br = _Branches(self.n_latent, self.res_index, self.dual and use_res and exstyles is not None, fuse_index, interp_weights)
        if br.modres or br.mixed:
            if exstyles.ndim < 3:
                res = self.e._mapping("generator.style.", exstyles).unsqueeze(1).repeat(1, self.n_latent, 1)
                ada = exstyles.unsqueeze(1).repeat(1, self.n_latent, 1)
            else:
                n, l, d = exstyles.shape
                res, ada = self.e._mapping("generator.style.", exstyles.reshape(n * l, d)).reshape(n, l, d), exstyles
            if br.mixed:
                from .eager import _equal_linear
                latent = latent.clone()
                for i in br.mixed:
                    t = _equal_linear(ada[:, i], sd[f"generator.res.{i}.weight"], sd[f"generator.res.{i}.bias"])
                    latent[:, i] = br.iw[i] * t + (1 - br.iw[i]) * latent[:, i]
        out = sd[g + "input.input"].repeat(b, 1, 1, 1)
        out = self._styled(out, latent[:, 0], g + "conv1.", False, noise[0])
        if 0 in br.modres:
            out = self._ada_res(out, res[:, 0], br.iw[0], 0)
        skip = self.e._to_rgb(out, latent[:, 1], g + "to_rgb1.", None)
        i = 1
        for lvl in range(self.log_size - 2):
            out = self._styled(out, latent[:, i], f"{g}convs.{2 * lvl}.", True, noise[i])
            if i in br.modres:
                out = self._ada_res(out, res[:, i], br.iw[i], i)
            out = self._styled(out, latent[:, i + 1], f"{g}convs.{2 * lvl + 1}.", False, noise[i + 1])
            if i + 1 in br.modres:
                out = self._ada_res(out, res[:, i + 1], br.iw[i + 1], i + 1)
            skip = self.e._to_rgb(out, latent[:, i + 2], f"{g}to_rgbs.{lvl}.", skip)
            i += 2
            if (return_feat and i > self.res_index) or i > return_feature_ind:
                return out, skip
        return skip, (latent0 if return_latents else None)   # the un-mixed latent, as the reference returns it


# ----------------------------------------------------------------------------------------------------------------------
class _GenPlan:
    def __init__(self):
        self.bufs: Dict[str, torch.Tensor] = {}
        self.ops: List[tuple] = []
        self.keep: list = []
        self.convs: list = []


class GeneratorEngine:
    """Generator.forward / DualStyleGAN.forward on the GPU: one launch plan per (batch, levels run, active ModRes blocks,
    noise batch per layer) over libvtoonify_amd.so, in the layout of VToonifyEngine (NHWC activations in the compute dtype,
    planar fp32 RGB skip, per-sample modulated weights from vt_modulate_weight_batch).

    A StyledConv is its conv launch without bias and activation (the up-sampling ones in the `up_fir` form) followed by ONE
    vt_noise_bias_act pass in place; ToRGB therefore always runs as its own thin conv (the fused ToRGB epilogue needs the
    activated tensor).  The mapping network, truncation, T_s and the path mix run before the plan on fresh tensors
    (vt_pixel_norm, vt_linear, vt_lerp_rows).  The forward never waits for the device.  Host scalars (the truncation psi, the
    interp_weights) reach the device as small tensors cached by value: a call with values seen before copies nothing from the
    host; the first call with new values makes one pageable host-to-device copy of at most 18 floats, whose cost on the host
    has not been measured.

    Memory: the engine holds an fp32 copy of the weights and up to MAX_PLANS plans (a plan = every activation of one forward
    plus the per-sample modulated weights: about 0.3 GB per sample at 1024^2 in bf16, twice that in fp32); `release()` drops
    the plans."""
    MAX_PLANS = 4

    def __init__(self, sd: Dict[str, torch.Tensor], dual: bool, size: int, dtype: torch.dtype, device, x3: bool = False,
                 res_index: int = 6, style_dim: int = 512):
        from .engine import VToonifyEngine
        self.dual, self.size, self.dtype, self.D = dual, size, dtype, style_dim
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.lib()
        if self.device.type != "cuda" and not _lib.is_emulation():
            raise _lib.VtError("GeneratorEngine needs a GPU device; modules on the CPU run EagerGenerator")
        self.dt = dt_code(dtype)
        self.x3 = bool(x3) and dtype == torch.float32
        self.dt_conv = K.VT_F32X3 if self.x3 else self.dt
        self.h16 = dtype in (torch.bfloat16, torch.float16)
        self.esz = 2 if self.h16 else 4
        self.tile_hints: Dict[str, int] = {}
        self._wstream: Dict[int, torch.Tensor] = {}
        self.log_size = int(math.log2(size))
        self.n_latent, self.num_layers = 2 * self.log_size - 2, 2 * (self.log_size - 2) + 1
        self.res_index = res_index // 2 * 2
        self.g = "generator.generator." if dual else "generator."
        self.sd = {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in sd.items()}
        self._plans: Dict[tuple, _GenPlan] = {}
        self._scalars: Dict[tuple, torch.Tensor] = {}
        self.last_plan: Optional[_GenPlan] = None     # the plan of the most recent forward (tools/generator_bench.py)
        # borrowed plan machinery (descriptor bookkeeping, split-K workspaces, op replay): the same code as the frame engine
        for nm in ("_op_conv", "_apply_hint", "_finalize_convs", "_run", "_buf"):
            setattr(self, nm, getattr(VToonifyEngine, nm).__get__(self))
        self.conv_signature, self._info = VToonifyEngine.conv_signature, VToonifyEngine._info
        self._pack_static()

    def _pack_static(self):
        sd, g, T = self.sd, self.g, self.dtype
        self.modw, self.rgb_bias, self.w = {}, {}, {}
        names = ["conv1", "to_rgb1"] + [f"convs.{i}" for i in range(2 * (self.log_size - 2))] + \
            [f"to_rgbs.{i}" for i in range(self.log_size - 2)]
        for nm in names:
            self.modw[nm] = sd[f"{g}{nm}.conv.weight"][0].contiguous()
            if nm.startswith("to_rgb"):
                self.rgb_bias[nm] = sd[f"{g}{nm}.bias"].reshape(3).contiguous()
        self.const = K.nchw_to_nhwc(sd[g + "input.input"], T)          # (1,4,4,C): every sample's conv1 reads it
        self.fir_rgb = sd[f"{g}to_rgbs.0.upsample.kernel"].contiguous()
        self.fir_up = sd[f"{g}convs.0.conv.blur.kernel"].contiguous()
        k = self.fir_up.detach().float().cpu()    # the LDS blur of the up_fir form is separable (as in VToonifyEngine)
        self.use_upblur = bool(k.shape == (4, 4) and float(k.sum()) != 0.0 and
                               torch.allclose(torch.outer(k.sum(1), k.sum(0)) / k.sum(), k, rtol=1e-5, atol=1e-7))
        if self.dual:
            i = 0
            while f"generator.res.{i}.conv.0.weight" in sd:
                for nm in ("conv", "conv2"):
                    w = sd[f"generator.res.{i}.{nm}.0.weight"]
                    self.w[f"res.{i}.{nm}"] = K.pack_conv_weight(w, scale=1.0 / math.sqrt(w.shape[1] * 9), out_dtype=T)
                i += 1

    # ------------------------------------------------------------------ front end: latents
    def _stream(self):
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(0)

    def _to(self, t):
        return t.detach().to(self.device, torch.float32).contiguous()

    def _mapping(self, prefix, z, n):
        x = K.pixel_norm(self._to(z).reshape(-1, z.shape[-1]))
        sc = (1.0 / math.sqrt(self.D)) * 0.01
        for i in range(1, n + 1):
            x = K.linear(x, self.sd[f"{prefix}{i}.weight"], self.sd[f"{prefix}{i}.bias"], sc, 0.01, ACT_LRELU, 0.2, SQRT2)
        return x.reshape(z.shape)

    def map_style(self, z):
        n = 1
        while f"{self.g}style.{n + 1}.weight" in self.sd:
            n += 1
        return self._mapping(self.g + "style.", z, n)

    def _truncate(self, s, t, psi):
        t = self._to(t)
        if t.numel() != s.shape[-1] and t.shape != s.shape:
            t = t.expand_as(s).contiguous()
        return lerp_rows(t, s, self._scalar_tensor((float(psi),)))

    def _scalar_tensor(self, values: tuple) -> torch.Tensor:
        """`values` as an fp32 tensor on the device, cached by value (at most 64 entries)."""
        t = self._scalars.get(values)
        if t is None:
            if len(self._scalars) >= 64:
                self._scalars.pop(next(iter(self._scalars)))
            t = self._scalars[values] = torch.tensor(values, dtype=torch.float32).to(self.device)
        return t

    def release(self):
        """Drop every cached plan (activations, modulated weights, noise buffers); the next forward builds its plan again."""
        self._plans.clear()
        self.last_plan = None

    # ------------------------------------------------------------------ the plan
    def _layers(self, n_levels):
        """(name, latent row, demodulate, upsample) of every modulated conv that runs."""
        out = [("conv1", 0, True, False), ("to_rgb1", 1, False, False)]
        for lvl in range(n_levels):
            out += [(f"convs.{2 * lvl}", 1 + 2 * lvl, True, True), (f"convs.{2 * lvl + 1}", 2 + 2 * lvl, True, False),
                    (f"to_rgbs.{lvl}", 3 + 2 * lvl, False, False)]
        return out

    def _build(self, B, n_levels, modres, nbs) -> _GenPlan:
        sd, g, lib, dt, esz, D, L = self.sd, self.g, self.lib, self.dt, self.esz, self.D, self.n_latent
        f32 = torch.float32
        plan = _GenPlan()
        ops = plan.ops
        lat = self._buf(plan, "latent", (B, L, D), f32)
        res = self._buf(plan, "resstyles", (B, L, D), f32)
        iw = self._buf(plan, "iw", (L,), f32)
        lins, mods, wm = [], [], {}

        def lin(y, ld_y, x, W, b, w_scale):
            it = _lib.LinearItem()
            it.y, it.x, it.W, it.b = K._ptr(y), K._ptr(x), W.data_ptr(), b.data_ptr()
            it.ld_y, it.ld_x, it.rows = ld_y, L * D, B
            it.out_dim, it.in_dim = W.shape
            it.act, it.w_scale, it.b_scale, it.slope, it.gain = ACT_NONE, w_scale, 1.0, 0.2, 1.0
            lins.append(it)

        for name, row, demod, up in self._layers(n_levels):
            w = self.modw[name]
            cout, cin, k, _ = w.shape
            s = self._buf(plan, f"s.{name}", (B, cin), f32)
            lin(s, cin, lat.data_ptr() + row * D * 4, sd[f"{g}{name}.conv.modulation.weight"],
                sd[f"{g}{name}.conv.modulation.bias"], 1.0 / math.sqrt(D))
            phases = 4 if (up and not self.use_upblur) else 1
            taps = 9 if up else k * k
            wm[name] = self._buf(plan, f"wm.{name}", (B, phases * cout, taps, cin))
            for b in range(B):
                it = _lib.ModulateItem()
                it.out = wm[name].data_ptr() + b * phases * cout * taps * cin * esz
                it.weight, it.s = w.data_ptr(), s.data_ptr() + b * cin * 4
                it.fir = self.fir_up.data_ptr() if (up and not self.use_upblur) else None
                it.cout, it.cin, it.k, it.demodulate = cout, cin, k, int(demod)
                it.scale = 1.0 / math.sqrt(cin * k * k)
                mods.append(it)
        for i in modres:     # AdaIN gamma / beta of the active ModRes blocks (dualstylegan.py:16-18), rows resstyles[:, i]
            for nm in ("norm", "norm2"):
                Wl = sd[f"generator.res.{i}.{nm}.style.weight"]
                gb = self._buf(plan, f"gb.{i}.{nm}", (B, Wl.shape[0]), f32)
                lin(gb, Wl.shape[0], res.data_ptr() + i * D * 4, Wl, sd[f"generator.res.{i}.{nm}.style.bias"], 1.0)
        arr = (_lib.LinearItem * len(lins))(*lins)
        marr = (_lib.ModulateItem * len(mods))(*mods)
        plan.keep += [arr, marr]
        ops.append((lib.vt_linear_batch, (arr, len(lins)), "linear_batch"))
        ops.append((lib.vt_modulate_weight_batch, (marr, len(mods), dt), "modulate_batch"))

        plan.noise = []

        def styled_tail(x, j, name, hw, c):
            nz = self._buf(plan, f"noise{j}", (nbs[j], hw), f32)
            plan.noise.append(nz)
            ops.append((lib.vt_noise_bias_act,
                        (C.c_void_p(x.data_ptr()), c, C.c_void_p(x.data_ptr()), c, C.c_void_p(nz.data_ptr()), nbs[j],
                         C.c_void_p(sd[f"{g}{name}.noise.weight"].data_ptr()), C.c_void_p(sd[f"{g}{name}.activate.bias"].data_ptr()),
                         B, hw, c, dt),
                        {"name": "noise_bias_act", "kernel": "noise_bias_act_kernel", "flops": 0, "bytes": 2 * B * hw * c * esz}))

        def mod_res(x, i, c, h, w):
            """AdaResBlock (dualstylegan.py:38-45): conv(AdaIN(x)) -> conv2(AdaIN(.)) * w_i + x, w_i read from device memory."""
            hw = h * w
            nrm, tmp, out = (self._buf(plan, f"mr{i}.{t}", (B, h, w, c)) for t in ("nrm", "tmp", "out"))

            def plane(dst, src, gb):
                ops.append((lib.vt_instnorm_plane,
                            (C.c_void_p(dst.data_ptr()), c, C.c_void_p(src.data_ptr()), c, C.c_void_p(0), 0, B, hw, c,
                             C.c_void_p(gb.data_ptr()), gb.shape[1], dt),
                            {"name": "adain", "kernel": "instnorm_plane", "flops": 0, "bytes": 2 * B * hw * c * esz}))
            kw = dict(c0=c, ld0=c, n=B, h=h, w=w, out_h=h, out_w=w, cout=c, kh=3, kw=3, pad=1, act=ACT_LRELU, gain=SQRT2, ld_out=c)
            plane(nrm, x, plan.bufs[f"gb.{i}.norm"])
            self._op_conv(ops, plan, src0=nrm, weight=self.w[f"res.{i}.conv"], bias=sd[f"generator.res.{i}.conv.1.bias"],
                          out=tmp, **kw)
            plane(tmp, tmp, plan.bufs[f"gb.{i}.norm2"])
            self._op_conv(ops, plan, src0=tmp, weight=self.w[f"res.{i}.conv2"], bias=sd[f"generator.res.{i}.conv2.1.bias"],
                          alpha_dev=iw.data_ptr() + 4 * i, beta=1.0, resid=x, ld_res=c, out=out, **kw)
            return out

        def to_rgb(x, name, c, h, w, rgb, resid):
            for b in range(B):
                ptr = rgb.data_ptr() + b * 3 * h * w * 4
                self._op_conv(ops, plan, src0=x.data_ptr() + b * h * w * c * esz, c0=c, ld0=c, n=1, h=h, w=w, out_h=h, out_w=w,
                              weight=wm[name][b], cout=3, kh=1, kw=1, bias=self.rgb_bias[name], out=ptr, ld_out=0,
                              out_layout=OUT_NCHW, out_dtype=K.VT_F32, **(dict(beta=1.0, resid=ptr) if resid else {}))

        h = w = 4
        c = self.modw["conv1"].shape[0]
        cur = self._buf(plan, "x.conv1", (B, h, w, c))
        for b in range(B):
            self._op_conv(ops, plan, src0=self.const, c0=c, ld0=c, n=1, h=h, w=w, out_h=h, out_w=w, weight=wm["conv1"][b],
                          cout=c, kh=3, kw=3, pad=1, out=cur.data_ptr() + b * h * w * c * esz, ld_out=c)
        styled_tail(cur, 0, "conv1", h * w, c)
        if 0 in modres:
            cur = mod_res(cur, 0, c, h, w)
        rgb = self._buf(plan, "rgb.4", (B, 3, h, w), f32)
        to_rgb(cur, "to_rgb1", c, h, w, rgb, False)
        i = 1
        for lvl in range(n_levels):
            n1, n2, n3 = f"convs.{2 * lvl}", f"convs.{2 * lvl + 1}", f"to_rgbs.{lvl}"
            co, hw = self.modw[n1].shape[0], h * w
            up = self._buf(plan, f"x.{n1}", (B, 2 * h, 2 * w, co))
            for b in range(B):
                src, dst = cur.data_ptr() + b * hw * c * esz, up.data_ptr() + b * 4 * hw * co * esz
                # the reference's MACs: conv_transpose2d (9 per input pixel) + the 4x4 blur (16 per output element)
                ref_macs = hw * c * co * 9 + 4 * hw * co * 16
                if self.use_upblur:
                    self._op_conv(ops, plan, ref_macs=ref_macs, src0=src, c0=c, ld0=c, n=1, h=h, w=w, out_h=2 * h, out_w=2 * w,
                                  weight=wm[n1][b], cout=co, kh=3, kw=3, up_fir=self.fir_up, out=dst, ld_out=co)
                else:
                    self._op_conv(ops, plan, ref_macs=ref_macs, src0=src, c0=c, ld0=c, n=1, h=h, w=w, out_h=h, out_w=w,
                                  weight=wm[n1][b], cout=co, kh=3, kw=3, pad=1, phases=4, out=dst, ld_out=co)
            h, w, c = 2 * h, 2 * w, co
            styled_tail(up, i, n1, h * w, c)
            if i in modres:
                up = mod_res(up, i, c, h, w)
            o2 = self._buf(plan, f"x.{n2}", (B, h, w, c))
            for b in range(B):
                off = b * h * w * c * esz
                self._op_conv(ops, plan, src0=up.data_ptr() + off, c0=c, ld0=c, n=1, h=h, w=w, out_h=h, out_w=w, weight=wm[n2][b],
                              cout=c, kh=3, kw=3, pad=1, out=o2.data_ptr() + off, ld_out=c)
            styled_tail(o2, i + 1, n2, h * w, c)
            if i + 1 in modres:
                o2 = mod_res(o2, i + 1, c, h, w)
            rgb2 = self._buf(plan, f"rgb.{h}", (B, 3, h, w), f32)
            # skip = Upsample(skip): upfirdn2d up=2 pad=(2,1) (model.py:32-50), fp32 planes
            ops.append((lib.vt_upfirdn2d,
                        (C.c_void_p(rgb2.data_ptr()), C.c_void_p(rgb.data_ptr()), C.c_void_p(self.fir_rgb.data_ptr()),
                         B * 3, h // 2, w // 2, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1, K.VT_F32),
                        {"name": "upfirdn2d", "kernel": "upfirdn2d", "flops": 0, "bytes": B * 3 * h * w * 5}))
            to_rgb(o2, n3, c, h, w, rgb2, True)
            cur, rgb = o2, rgb2
            i += 2
        plan.image, plan.feat = rgb, (cur, c, h, w)
        self._finalize_convs(plan)
        return plan

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, styles, exstyles=None, return_latents=False, return_feat=False, inject_index=None, truncation=1,
                truncation_latent=None, input_is_latent=False, noise=None, randomize_noise=True, z_plus_latent=False,
                use_res=True, fuse_index=18, interp_weights=(1,) * 18, return_feature_ind=999):
        sd, L, D = self.sd, self.n_latent, self.D
        _check_styles(styles, input_is_latent, z_plus_latent)
        latent = _assemble_latent([self._to(s) for s in styles], L, inject_index, truncation, truncation_latent,
                                  input_is_latent, self.map_style, self._truncate)
        B, latent0 = latent.shape[0], latent
        br = _Branches(L, self.res_index, self.dual and use_res and exstyles is not None, fuse_index, interp_weights)
        n_levels, early = self.log_size - 2, False
        for lvl in range(self.log_size - 2):
            i = 3 + 2 * lvl
            if (return_feat and i > self.res_index) or i > return_feature_ind:
                n_levels, early = lvl + 1, True
                break
        n_noise = 1 + 2 * n_levels
        if noise is not None:
            noise = [self._to(t) for t in list(noise)[:n_noise]]
            nbs = tuple(int(t.shape[0]) for t in noise)
        else:
            nbs = (B if randomize_noise else 1,) * n_noise
        modres = tuple(i for i in br.modres if i <= 2 * n_levels)
        key = (B, n_levels, modres, nbs)
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= self.MAX_PLANS:
                self._plans.pop(next(iter(self._plans)))
            plan = self._plans[key] = self._build(B, n_levels, modres, nbs)
        self.last_plan = plan
        if br.modres or br.mixed:
            ex = self._to(exstyles)
            n_tc = 1
            while f"generator.style.{n_tc + 1}.weight" in sd:
                n_tc += 1
            r = self._mapping("generator.style.", ex, n_tc)
            plan.bufs["resstyles"].copy_(r.unsqueeze(1).expand(B, L, D) if ex.ndim < 3 else r)
            if br.mixed:
                latent = latent.clone()
                iw_dev = self._scalar_tensor(tuple(br.iw))
                for i in br.mixed:
                    x, ld = (ex, D) if ex.ndim < 3 else (ex[:, i], L * D)
                    t = K.linear(x, sd[f"generator.res.{i}.weight"], sd[f"generator.res.{i}.bias"], 1.0 / math.sqrt(D), 1.0,
                                 ld_x=ld, rows=B)
                    latent[:, i] = lerp_rows(latent[:, i].contiguous(), t, iw_dev[i:i + 1])
            plan.bufs["iw"].copy_(self._scalar_tensor(tuple(br.iw))[:L])
        plan.bufs["latent"].copy_(latent)
        if noise is not None:
            for nz, t in zip(plan.noise, noise):
                nz.copy_(t.reshape(nz.shape))
        elif randomize_noise:
            key64 = draw_key()
            for j, nz in enumerate(plan.noise):
                randn_into(nz, key64, j)
        else:
            for j, nz in enumerate(plan.noise):
                nz.copy_(sd[f"{self.g}noises.noise_{j}"].reshape(nz.shape))
        self._run(plan.ops, self._stream())
        if early:
            x, c, h, w = plan.feat
            return K.nhwc_to_nchw(x, c, B, c, h, w, self.dtype, torch.float32, self.device, x), plan.image.clone()
        return plan.image.clone(), (latent0 if return_latents else None)

    def run_ops(self, ops):
        """Replay a subset of a plan's ops on the current stream (tools/generator_bench.py: the noise passes alone)."""
        self._run(ops, self._stream())


# ----------------------------------------------------------------------------------------------------------------------
from .vtoonify import _DualStyleGAN, _StyleGAN2   # noqa: E402  (vtoonify.py imports this module lazily: no cycle)


class _Forward:
    """What Generator and DualStyleGAN share: the executor behind `forward` and the noise / latent helpers of the reference.

    compute_dtype / exact_fp32 follow the owning VToonify (fp32 with the products as three bf16 MFMAs by default, fp32_exact,
    bf16, fp16); a module built on its own takes the same defaults and may set the two attributes before its first call."""
    compute_dtype = torch.float32
    exact_fp32 = False
    _dual = False

    def _prefixed(self):
        return {"generator." + k: v for k, v in self.state_dict().items()}

    def _fingerprint(self):
        h = 0
        for t in list(self.parameters()) + list(self.buffers()):
            h = (h * 1000003 + t.data_ptr() * 31 + t._version) & 0xFFFFFFFFFFFFFFF
        return (h, self.compute_dtype, self.exact_fp32)

    def executor(self):
        """EagerGenerator for parameters on the CPU, else the (cached) GeneratorEngine; a weight load, an in-place edit or a
        move of any parameter builds a new engine."""
        dev = next(self.parameters()).device
        res_index = getattr(self, "res_index", 6)
        if _host_device(dev):
            return EagerGenerator(self._prefixed(), self._dual, self.size, res_index)
        fp = self._fingerprint()
        cached = self.__dict__.get("_gen_engine")
        if cached is None or cached[0] != fp:
            eng = GeneratorEngine(self._prefixed(), self._dual, self.size, self.compute_dtype, dev,
                                  x3=self.compute_dtype == torch.float32 and not self.exact_fp32, res_index=res_index,
                                  style_dim=self.style_dim)
            cached = self.__dict__["_gen_engine"] = (fp, eng)
        return cached[1]

    def release_engine(self):
        """Drop this module's GeneratorEngine (its fp32 weight copy and its plans); the next call builds it again."""
        self.__dict__.pop("_gen_engine", None)

    def _stylegan(self):
        return self.generator if self._dual else self

    def make_noise(self):
        device = self._stylegan().input.input.device
        noises = [torch.randn(1, 1, 2 ** 2, 2 ** 2, device=device)]
        for i in range(3, self.log_size + 1):
            for _ in range(2):
                noises.append(torch.randn(1, 1, 2 ** i, 2 ** i, device=device))
        return noises

    def draw_noise(self, batch: int):
        """Exactly the list of maps that a `forward(..., randomize_noise=True)` of `batch` samples made at the same state of
        torch's default CPU generator would draw: (batch,1,H_i,W_i) fp32, Philox4x32-10 + Box-Muller under one 64-bit key per
        call (include/vtoonify_amd_generator.h).  Statistically N(0,1); NOT the bits of torch's `normal_`."""
        device = self._stylegan().input.input.device
        if _host_device(device):
            key = draw_key()
            return [_randn_host(batch * h * w, key, i).view(batch, 1, h, w) for i, (h, w) in enumerate(noise_sizes(self.size))]
        return draw_noise(batch, self.size, device)

    def get_latent(self, input):
        with torch.no_grad():
            return self._stylegan().executor().map_style(input)

    def mean_latent(self, n_latent):
        latent_in = torch.randn(n_latent, self.style_dim, device=self._stylegan().input.input.device)
        return self.get_latent(latent_in).mean(0, keepdim=True)


class Generator(_Forward, _StyleGAN2):
    """StyleGAN2 generator with the reference's constructor, state_dict schema and forward (model/stylegan/model.py:395-590).
    `blur_kernel` other than [1, 3, 3, 1] and `lr_mlp` other than 0.01 are not supported (the reference never passes them)."""

    def __init__(self, size, style_dim, n_mlp, channel_multiplier=2, blur_kernel=[1, 3, 3, 1], lr_mlp=0.01):
        if list(blur_kernel) != [1, 3, 3, 1] or lr_mlp != 0.01:
            raise NotImplementedError("Generator: blur_kernel [1, 3, 3, 1] and lr_mlp 0.01 only")
        super().__init__(size, style_dim, n_mlp, channel_multiplier)

    def forward(self, styles, return_latents=False, inject_index=None, truncation=1, truncation_latent=None,
                input_is_latent=False, noise=None, randomize_noise=True, z_plus_latent=False, return_feature_ind=999):
        """Randomised noise is drawn by the package's own counter-based generator, seeded from torch's default CPU generator
        (see `draw_noise`): `torch.manual_seed` reproduces a call, but the maps are not the bits of torch's `normal_`."""
        with torch.no_grad():
            return self.executor().forward(styles, None, return_latents=return_latents, inject_index=inject_index,
                                           truncation=truncation, truncation_latent=truncation_latent,
                                           input_is_latent=input_is_latent, noise=noise, randomize_noise=randomize_noise,
                                           z_plus_latent=z_plus_latent, use_res=False, return_feature_ind=return_feature_ind)


class DualStyleGAN(_Forward, _DualStyleGAN):
    """DualStyleGAN with the reference's constructor, state_dict schema and forward (model/dualstylegan.py:47-200)."""
    _dual = True
    _stylegan_cls = Generator

    def __init__(self, size, style_dim, n_mlp, channel_multiplier=2, twoRes=True, res_index=6):
        super().__init__(size, style_dim, n_mlp, channel_multiplier, res_index)
        self.res_index = res_index // 2 * 2

    def _prefixed(self):
        return {"generator." + k: v for k, v in self.state_dict().items()}

    def forward(self, styles, exstyles, return_latents=False, return_feat=False, inject_index=None, truncation=1,
                truncation_latent=None, input_is_latent=False, noise=None, randomize_noise=True, z_plus_latent=False,
                use_res=True, fuse_index=18, interp_weights=[1] * 18):
        """Randomised noise: see `Generator.forward`."""
        with torch.no_grad():
            return self.executor().forward(styles, exstyles, return_latents=return_latents, return_feat=return_feat,
                                           inject_index=inject_index, truncation=truncation,
                                           truncation_latent=truncation_latent, input_is_latent=input_is_latent, noise=noise,
                                           randomize_noise=randomize_noise, z_plus_latent=z_plus_latent, use_res=use_res,
                                           fuse_index=fuse_index, interp_weights=interp_weights)
