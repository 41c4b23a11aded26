"""pSp style encoder (GradualStyleEncoder) on the MI355X kernels -- SURVEY.md section 8 row a17.

Reference: model/encoder/encoders/psp_encoders.py:35-116 (IR-SE-50 trunk, FPN taps at body
6/20/23, 18 map2style heads) and helpers.py:53-119 (bottleneck_IR_SE, SEModule); constructed and
loaded by util.load_psp_standalone (util.py:143-161).  It runs ONCE per video/image
(style_transfer.py:143,210), 145 GFLOP at 3x256x256.

`GradualStyleEncoder` below keeps the reference's constructor and state_dict schema (621 entries
for (50, 'ir_se')) so `psp.load_state_dict({k[len('encoder.'):]: v ...})` works unchanged; the
arithmetic runs in `PspEngine`, a static launch plan over libvtoonify_amd.so:
  * every Conv2d is one vt_conv2d launch (direct-to-LDS MFMA kernels), with the FOLLOWING eval-mode
    BatchNorm folded into its weights/bias at load time, PReLU / LeakyReLU(0.01) fused in the
    epilogue (per-channel slopes: vt_conv_desc.slope_vec);
  * a BatchNorm that PRECEDES a zero-padded conv cannot be folded (the border would see the
    shift): it is one vt_affine_apply pass;
  * SE block: vt_channel_mean -> two vt_linear (ReLU, sigmoid) -> vt_se_apply, which also adds the
    shortcut (MaxPool2d(1, stride) = strided read);
  * FPN: 1x1 lateral convs + vt_upsample_bilinear_add;  heads: stride-2 convs + EqualLinear.
There is no eager-PyTorch fallback; weight folding at load time is parameter preprocessing.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from . import kernels as K
from ._lib import ACT_LRELU, ACT_NONE, ACT_SIGMOID

BLOCKS_50 = [(64, 64, 3), (64, 128, 4), (128, 256, 14), (256, 512, 3)]  # helpers.py:33-39
BN_EPS = 1e-5


def ir_units(num_layers: int = 50):
    if num_layers != 50:
        raise NotImplementedError("only the IR-SE-50 trunk used by util.load_psp_standalone is built")
    out = []
    for cin, depth, n in BLOCKS_50:
        out.append((cin, depth, 2))
        out += [(depth, depth, 1)] * (n - 1)
    return out


# ------------------------------------------------------------------------- parameter schema
def _bn(c):
    return nn.BatchNorm2d(c)


class _SE(nn.Module):
    def __init__(self, c, r):
        super().__init__()
        self.fc1 = nn.Conv2d(c, c // r, 1, bias=False)
        self.fc2 = nn.Conv2d(c // r, c, 1, bias=False)


class _Bottleneck(nn.Module):
    def __init__(self, cin, depth, stride):
        super().__init__()
        if cin != depth:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(cin, depth, 1, stride, bias=False), _bn(depth))
        else:
            self.shortcut_layer = nn.Identity()  # MaxPool2d(1, stride): no parameters
        self.res_layer = nn.Sequential(_bn(cin), nn.Conv2d(cin, depth, 3, 1, 1, bias=False), nn.PReLU(depth),
                                       nn.Conv2d(depth, depth, 3, stride, 1, bias=False), _bn(depth),
                                       _SE(depth, 16))


class _P(nn.Module):
    def __init__(self, **params):
        super().__init__()
        for k, v in params.items():
            self.register_parameter(k, nn.Parameter(v))


class _StyleBlock(nn.Module):
    def __init__(self, in_c, out_c, spatial):
        super().__init__()
        n = int(math.log2(spatial))
        mods = []
        for i in range(n):
            mods += [nn.Conv2d(in_c if i == 0 else out_c, out_c, 3, 2, 1), nn.Identity()]
        self.convs = nn.Sequential(*mods)
        self.linear = _P(weight=torch.randn(out_c, out_c), bias=torch.zeros(out_c))  # EqualLinear lr_mul=1
        self.spatial = spatial


class GradualStyleEncoder(nn.Module):
    """Same constructor / state_dict / forward contract as the reference class."""

    def __init__(self, num_layers=50, mode="ir_se", opts=None, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if mode != "ir_se":
            raise NotImplementedError("only mode='ir_se' (what util.load_psp_standalone builds)")
        opts = opts or argparse.Namespace(input_nc=3, n_styles=18)
        self.input_nc = int(getattr(opts, "input_nc", 3))
        self.style_count = int(getattr(opts, "n_styles", 18))
        self.coarse_ind, self.middle_ind = 3, 7
        self.compute_dtype = compute_dtype
        self.input_layer = nn.Sequential(nn.Conv2d(self.input_nc, 64, 3, 1, 1, bias=False), _bn(64), nn.PReLU(64))
        self.body = nn.Sequential(*[_Bottleneck(*u) for u in ir_units(num_layers)])
        self.styles = nn.ModuleList()
        for i in range(self.style_count):
            sp = 16 if i < self.coarse_ind else 32 if i < self.middle_ind else 64
            self.styles.append(_StyleBlock(512, 512, sp))
        self.latlayer1 = nn.Conv2d(256, 512, 1)
        self.latlayer2 = nn.Conv2d(128, 512, 1)
        self._engine: Optional[PspEngine] = None
        self.latent_avg: Optional[torch.Tensor] = None   # util.py:155-160 adds it in a forward hook
        self.requires_grad_(False)
        self.eval()

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._engine = None
        return super().load_state_dict(*a, **k)

    def engine(self) -> "PspEngine":
        if self._engine is None:
            dev = next(self.parameters()).device
            self._engine = PspEngine(self.state_dict(), self.style_count, self.compute_dtype, dev)
        return self._engine

    def forward(self, x):
        y = self.engine().forward(x)
        if self.latent_avg is not None:
            y = y + self.latent_avg.to(y).repeat(y.shape[0], 1, 1)
        return y


# ------------------------------------------------------------------------------- the engine
class PspEngine:
    def __init__(self, state_dict: Dict[str, torch.Tensor], n_styles: int = 18,
                 dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None):
        assert dtype in (torch.bfloat16, torch.float16, torch.float32)
        self.dtype, self.dt = dtype, K.dt_code(dtype)
        self.esz = torch.empty((), dtype=dtype).element_size()
        self.device = device or next(iter(state_dict.values())).device
        if self.device.type != "cuda" and not _lib.is_emulation():
            raise _lib.VtError("PspEngine needs a GPU device (no CPU path)")
        self.lib = _lib.lib()
        self.n_styles = n_styles
        self.sd = {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in state_dict.items()
                   if v.dtype.is_floating_point}
        self.units = ir_units(50)
        self._plans: Dict[tuple, dict] = {}
        self._pack()

    # -- load-time parameter preprocessing ------------------------------------------------
    def _bn_affine(self, prefix):
        sd = self.sd
        scale = sd[prefix + "weight"] / torch.sqrt(sd[prefix + "running_var"] + BN_EPS)
        return scale.contiguous(), (sd[prefix + "bias"] - sd[prefix + "running_mean"] * scale).contiguous()

    def _pack(self):
        sd, T = self.sd, self.dtype
        self.w: Dict[str, torch.Tensor] = {}
        self.b: Dict[str, torch.Tensor] = {}

        def conv_bn(wkey, bnprefix):   # conv followed by BatchNorm: fold
            sc, sh = self._bn_affine(bnprefix)
            w = sd[wkey] * sc.reshape(-1, 1, 1, 1)
            return K.pack_conv_weight(w.contiguous(), out_dtype=T), sh

        self.w["in"], self.b["in"] = conv_bn("input_layer.0.weight", "input_layer.1.")
        for i, (cin, depth, stride) in enumerate(self.units):
            p = f"body.{i}."
            self.w[p + "c1"] = K.pack_conv_weight(sd[p + "res_layer.1.weight"], out_dtype=T)
            self.w[p + "c2"], self.b[p + "c2"] = conv_bn(p + "res_layer.3.weight", p + "res_layer.4.")
            if cin != depth:
                self.w[p + "sc"], self.b[p + "sc"] = conv_bn(p + "shortcut_layer.0.weight", p + "shortcut_layer.1.")
            self.b[p + "bn0"] = self._bn_affine(p + "res_layer.0.")
        for j in range(self.n_styles):
            p = f"styles.{j}."
            i = 0
            while p + f"convs.{2 * i}.weight" in sd:
                self.w[p + f"c{i}"] = K.pack_conv_weight(sd[p + f"convs.{2 * i}.weight"], out_dtype=T)
                i += 1
        self.w["lat1"] = K.pack_conv_weight(sd["latlayer1.weight"], out_dtype=T)
        self.w["lat2"] = K.pack_conv_weight(sd["latlayer2.weight"], out_dtype=T)

    # -- plan ------------------------------------------------------------------------------
    def _build(self, B, H, W):
        sd, lib, dt, T = self.sd, self.lib, self.dt, self.dtype
        dev, f32 = self.device, torch.float32
        plan = {"ops": [], "keep": [], "bufs": {}, "convs": []}
        ops, keep, bufs = plan["ops"], plan["keep"], plan["bufs"]

        def buf(name, shape, dtype=None):
            t = torch.empty(shape, dtype=dtype or T, device=dev)
            bufs[name] = t
            return t

        def conv(**kw):
            d = K.make_conv_desc(dtype=dt, **kw)
            keep.append(d)
            plan["convs"].append(d)
            ops.append((lib.vt_conv2d, (C.byref(d),)))

        def rep(v):  # per-channel vector -> [B][c] (the affine kernels index by image)
            return v.reshape(1, -1).repeat(B, 1).contiguous()

        x_in = buf("x_in", (B, self.sd["input_layer.0.weight"].shape[1], H, W), f32)
        cin0 = x_in.shape[1]
        x0 = buf("x0", (B, H, W, (cin0 + 7) // 8 * 8))
        ops.append((lib.vt_nchw_to_nhwc, (C.c_void_p(x0.data_ptr()), x0.shape[-1], C.c_void_p(x_in.data_ptr()), B,
                                          cin0, H * W, K.VT_F32, dt)))
        cur = buf("a_in", (B, H, W, 64))
        conv(src0=x0, c0=x0.shape[-1], ld0=x0.shape[-1], n=B, h=H, w=W, out_h=H, out_w=W, weight=self.w["in"],
             cout=64, kh=3, kw=3, pad=1, bias=self.b["in"], act=ACT_LRELU, slope_vec=sd["input_layer.2.weight"],
             out=cur, ld_out=64)
        h, w = H, W
        taps = {}
        ws_bytes = 0
        for i, (cin, depth, stride) in enumerate(self.units):
            p = f"body.{i}."
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            sc0, sh0 = self.b[p + "bn0"]
            s_sc, s_sh = rep(sc0), rep(sh0)
            keep += [s_sc, s_sh]
            t0 = buf(p + "t0", (B, h, w, cin))
            ops.append((lib.vt_affine_apply, (C.c_void_p(t0.data_ptr()), cin, C.c_void_p(cur.data_ptr()), cin,
                                              C.c_void_p(0), 0, C.c_void_p(s_sc.data_ptr()),
                                              C.c_void_p(s_sh.data_ptr()), B, h * w, cin, dt)))
            t1 = buf(p + "t1", (B, h, w, depth))
            conv(src0=t0, c0=cin, ld0=cin, n=B, h=h, w=w, out_h=h, out_w=w, weight=self.w[p + "c1"], cout=depth,
                 kh=3, kw=3, pad=1, act=ACT_LRELU, slope_vec=sd[p + "res_layer.2.weight"], out=t1, ld_out=depth)
            t2 = buf(p + "t2", (B, ho, wo, depth))
            conv(src0=t1, c0=depth, ld0=depth, n=B, h=h, w=w, out_h=ho, out_w=wo, weight=self.w[p + "c2"],
                 cout=depth, kh=3, kw=3, stride=stride, pad=1, bias=self.b[p + "c2"], out=t2, ld_out=depth)
            # SE gate
            mean = buf(p + "mean", (B, depth), f32)
            nb = max(K.instnorm_ws_bytes(B, ho * wo, depth), 16)
            ws_bytes = max(ws_bytes, nb)
            g1 = buf(p + "g1", (B, depth // 16), f32)
            gate = buf(p + "gate", (B, depth), f32)
            ops.append(("mean", (mean, t2, depth, B, ho * wo, depth)))
            fc1 = sd[p + "res_layer.5.fc1.weight"].reshape(depth // 16, depth).contiguous()
            fc2 = sd[p + "res_layer.5.fc2.weight"].reshape(depth, depth // 16).contiguous()
            keep += [fc1, fc2]
            ops.append((lib.vt_linear, (C.c_void_p(g1.data_ptr()), depth // 16, C.c_void_p(mean.data_ptr()), depth,
                                        C.c_void_p(fc1.data_ptr()), C.c_void_p(0), B, depth, depth // 16, 1.0, 1.0,
                                        ACT_LRELU, 0.0, 1.0)))       # ReLU
            ops.append((lib.vt_linear, (C.c_void_p(gate.data_ptr()), depth, C.c_void_p(g1.data_ptr()), depth // 16,
                                        C.c_void_p(fc2.data_ptr()), C.c_void_p(0), B, depth // 16, depth, 1.0, 1.0,
                                        ACT_SIGMOID, 0.0, 1.0)))
            # shortcut
            if cin != depth:
                scb = buf(p + "sc", (B, ho, wo, depth))
                conv(src0=cur, c0=cin, ld0=cin, n=B, h=h, w=w, out_h=ho, out_w=wo, weight=self.w[p + "sc"], cout=depth,
                     kh=1, kw=1, stride=stride, pad=0, bias=self.b[p + "sc"], out=scb, ld_out=depth)
                sc_t, sc_h, sc_w, sc_s = scb, ho, wo, 1
            else:
                sc_t, sc_h, sc_w, sc_s = cur, h, w, stride
            out = buf(p + "out", (B, ho, wo, depth))
            ops.append((lib.vt_se_apply, (C.c_void_p(out.data_ptr()), C.c_void_p(t2.data_ptr()),
                                          C.c_void_p(gate.data_ptr()), C.c_void_p(sc_t.data_ptr()), B, ho, wo, depth,
                                          sc_h, sc_w, sc_s, dt)))
            cur, h, w = out, ho, wo
            if i in (6, 20, 23):
                taps[i] = (cur, depth, h, w)
        plan["taps"] = taps
        (c1, _, h1, w1), (c2, _, h2, w2), (c3, _, h3, w3) = taps[6], taps[20], taps[23]
        # FPN (psp_encoders.py:106-112)
        l1 = buf("lat1", (B, h2, w2, 512))
        conv(src0=c2, c0=256, ld0=256, n=B, h=h2, w=w2, out_h=h2, out_w=w2, weight=self.w["lat1"], cout=512, kh=1, kw=1,
             bias=sd["latlayer1.bias"], out=l1, ld_out=512)
        p2 = buf("p2", (B, h2, w2, 512))
        ops.append((lib.vt_upsample_bilinear_add, (C.c_void_p(p2.data_ptr()), C.c_void_p(c3.data_ptr()),
                                                   C.c_void_p(l1.data_ptr()), B, h3, w3, h2, w2, 512, dt)))
        l2 = buf("lat2", (B, h1, w1, 512))
        conv(src0=c1, c0=128, ld0=128, n=B, h=h1, w=w1, out_h=h1, out_w=w1, weight=self.w["lat2"], cout=512, kh=1, kw=1,
             bias=sd["latlayer2.bias"], out=l2, ld_out=512)
        p1 = buf("p1", (B, h1, w1, 512))
        ops.append((lib.vt_upsample_bilinear_add, (C.c_void_p(p1.data_ptr()), C.c_void_p(p2.data_ptr()),
                                                   C.c_void_p(l2.data_ptr()), B, h2, w2, h1, w1, 512, dt)))
        # map2style heads (psp_encoders.py:11-32, 102-112)
        out_codes = buf("codes", (B, self.n_styles, 512), f32)
        for j in range(self.n_styles):
            p = f"styles.{j}."
            src, hh, ww = (c3, h3, w3) if j < 3 else (p2, h2, w2) if j < 7 else (p1, h1, w1)
            i = 0
            while p + f"c{i}" in self.w:
                last = p + f"c{i + 1}" not in self.w
                ho, wo = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
                dst = buf(p + f"a{i}", (B, ho, wo, 512), f32 if last else None)
                conv(src0=src, c0=512, ld0=512, n=B, h=hh, w=ww, out_h=ho, out_w=wo, weight=self.w[p + f"c{i}"],
                     cout=512, kh=3, kw=3, stride=2, pad=1, bias=sd[p + f"convs.{2 * i}.bias"], act=ACT_LRELU,
                     slope=0.01, out=dst, ld_out=512, out_dtype=K.VT_F32 if last else None)
                src, hh, ww = dst, ho, wo
                i += 1
            if hh != 1 or ww != 1:
                raise _lib.VtError(f"input {H}x{W} too large for the map2style heads (x.view(-1, 512) needs 1x1)")
            ops.append((lib.vt_linear, (C.c_void_p(out_codes.data_ptr() + j * 512 * 4), self.n_styles * 512,
                                        C.c_void_p(src.data_ptr()), 512, C.c_void_p(sd[p + "linear.weight"].data_ptr()),
                                        C.c_void_p(sd[p + "linear.bias"].data_ptr()), B, 512, 512,
                                        1.0 / math.sqrt(512), 1.0, ACT_NONE, 0.0, 1.0)))
        # shared workspaces: instnorm partials (channel means) and split-K
        part = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        bufs["partials"] = part
        need = 0
        for d in plan["convs"]:
            need = max(need, int(lib.vt_conv2d_ws_bytes(C.byref(d))))
        if need:
            ws = torch.zeros((need,), dtype=torch.uint8, device=dev)
            bufs["splitk_ws"] = ws
            for d in plan["convs"]:
                d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), need
        plan["codes"] = out_codes
        plan["graph"] = None
        return plan

    def _stream(self):
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(0)

    def _launch(self, plan):
        st = self._stream()
        part = plan["bufs"]["partials"]
        for fn, args in plan["ops"]:
            if fn == "mean":
                mean, x, ld, n, hw, c = args
                rc = self.lib.vt_channel_mean(C.c_void_p(mean.data_ptr()), C.c_void_p(x.data_ptr()), ld, n, hw, c,
                                              C.c_void_p(part.data_ptr()), self.dt, st)
            else:
                rc = fn(*args, st)
            if rc != 0:
                raise _lib.VtError(f"pSp plan op failed (code {rc}): {self.lib.vt_last_error().decode()}")

    @torch.no_grad()
    def forward(self, x: torch.Tensor, use_graph: bool = False, taps: bool = False):
        B, c, H, W = x.shape
        key = (B, H, W)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._build(B, H, W)
            self._plans[key] = plan
        plan["bufs"]["x_in"].copy_(x.detach())
        if use_graph and self.device.type == "cuda":
            if plan["graph"] is None:
                self._launch(plan)
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._launch(plan)
                plan["graph"] = g
            plan["graph"].replay()
        else:
            self._launch(plan)
        y = plan["codes"].clone()
        if taps:
            res = {}
            for i, (t, cch, h, w) in plan["taps"].items():
                res[i] = K.nhwc_to_nchw(t, cch, B, cch, h, w, self.dtype, torch.float32, self.device, t)
            return y, res
        return y

    __call__ = forward
