"""Whole-frame executor for VToonify.forward on MI355X.

Restates the data flow of the reference's VToonify.forward (model/vtoonify.py:210-277) as a
static launch plan over libvtoonify_amd.so:

  * activations live in HBM as NHWC (channels innermost, padded to 8) in the compute dtype
    (bf16 for throughput, fp32 for parity); RGB skip images stay planar fp32;
  * every conv is one MFMA implicit-GEMM launch with its bias / LeakyReLU / residual /
    style-degree scaling fused in the epilogue; torch.cat never materialises (two-source
    loader); AdaIN in the ModRes blocks is a per-channel affine applied in the conv loader;
  * conv_transpose2d(stride 2) + 4x4 FIR blur of the up-sampling StyledConv collapses into
    one 3x3 conv with 4*Cout polyphase filters and a pixel-shuffle store
    (model/stylegan/model.py:273-286; derivation in DESIGN.md);
  * everything that depends only on (style, d_s) -- T_c/T_s linears, modulation,
    demodulated weights, AdaIN gamma/beta -- is recomputed on the GPU by the "style" op
    list; it can be cached per style tensor (off by default in the benchmark);
  * a plan is a flat list of (C function, prebuilt ctypes args): replaying it costs one
    foreign call per kernel, and it is hipGraph-capturable (no allocation, no sync).

Nothing here touches the CPU oracle; there is no eager-PyTorch compute path.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from . import kernels as K
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU_TANH, OUT_NCHW, OUT_NHWC

SQRT2 = math.sqrt(2.0)
N_LATENT = 18
_DIL = {1: 4, 2: 4, 3: 2, 4: 2, 5: 1, 6: 1}  # model/vtoonify.py:201-207
# header of fusion_skip's K range [skip(3) | zeros | f_E * m_E]: 64 channels, the layout of its packed weights (a whole number
# of K steps in every type).  The fused gate (VToonifyEngine(fused_gate=True), the default) forms the header in the conv's
# loader (vt_conv2d_hdr); only fused_gate=False still writes it to memory in front of f_E * m_E (vt_fusion_pack).
SKIP_HDR = 64


def _pad8(c: int) -> int:
    return (c + 7) // 8 * 8


class _Plan:
    def __init__(self):
        self.bufs: Dict[str, torch.Tensor] = {}
        self.style_ops: List[Tuple] = []
        self.enc_ops: List[Tuple] = []
        self.gen_ops: List[Tuple] = []
        self.keep: list = []          # ctypes objects that must outlive the plan
        self.masks: List[torch.Tensor] = []
        self.graphs: dict = {}        # with_style -> torch.cuda.CUDAGraph
        self.convs: list = []         # (ConvDesc, info) of every conv launch


class VToonifyEngine:
    """Inference engine bound to one device and one set of weights.

    state_dict: the reference's `g_ema` schema, fp32, on `device`.
    dtype: torch.bfloat16 (fast), torch.float16 (the kernels and plans of bf16 at 0.98x its frame rate, three more mantissa bits: close to the reference's
    quality; range up to 65504) or torch.float32 (parity mode, exact-fp32 MFMA).
    x3 (fp32 only): the convolutions run as three bf16 MFMAs per fp32 product (vt_conv_desc.dtype = VT_F32X3: operands split
    into bf16 head + remainder in the fragment registers, fp32 accumulate) -- every tensor, weight and non-conv kernel stays
    fp32.  4e-5 of max|y| against the fp32 oracle (bar 1e-4) instead of 5e-6; the reference's precision at several times
    the speed of the exact-fp32 matrix instructions.
    """
    supports_borrow = True   # forward(..., borrow=True) hands out the plan's output buffer instead of a copy

    def __init__(self, state_dict: Dict[str, torch.Tensor], backbone: str = "dualstylegan",
                 in_size: int = 256, dtype: torch.dtype = torch.bfloat16,
                 device: Optional[torch.device] = None, cache_styles: bool = False,
                 tile_hints: Optional[Dict[str, int]] = None, style_gate: bool = False, x3: bool = False,
                 fuse_rgb128: bool = True, fused_gate=True, fold_rgb_up: bool = True):
        assert backbone in ("dualstylegan", "toonify")
        assert dtype in (torch.bfloat16, torch.float16, torch.float32)
        self.backbone = backbone
        self.dual = backbone == "dualstylegan"
        self.in_size = in_size
        self.dtype = dtype
        self.dt = K.dt_code(dtype)
        self.x3 = bool(x3) and dtype == torch.float32
        self.dt_conv = K.VT_F32X3 if self.x3 else self.dt   # vt_conv_desc.dtype; everything else sees self.dt
        self.h16 = dtype in (torch.bfloat16, torch.float16)   # 16-bit activations and weights: the same plans for either type
        self.precision = ({torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype] if self.h16 else
                          ("fp32x3" if self.x3 else "fp32_exact"))
        self.esz = 2 if self.h16 else 4
        any_t = next(iter(state_dict.values()))
        self.device = torch.device(device) if device is not None else any_t.device
        if self.device.type == "cuda" and self.device.index is None:   # "cuda" == the current device
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.lib()
        if self.device.type != "cuda" and not _lib.is_emulation():
            raise _lib.VtError("VToonifyEngine needs a GPU device (no CPU path)")
        self.cache_styles = cache_styles
        self.fuse_rgb128 = bool(fuse_rgb128)
        # fused_gate: the Fusion levels without the packed operand [skip | zeros | f_E * m_E]: the mask conv writes
        # f_E * m_E itself (vt_conv2d_gate) and fusion_skip reads the skip planes as a second source (vt_conv2d_hdr).  Bit-identical
        # to `fused_gate=False`, which keeps the vt_fusion_pack launch and the 64-channel header for A/B measurements and tests.
        # True fuses a level where that measured faster (profiles/fusion_gate_fem.txt): every level without a mask (Toonify: the pack
        # pass just disappears), from 8192 pixels per image up with one (the mask conv's re-read of f_E and the header formed in
        # the loader cost what the pack pass took at 64^2 and below: 39.1 against 39.0 us, 32.8 against 32.2).  "all": every level
        # (tests, A/B).  Both forms give the same bits, so the rule is free to look at the geometry.
        self.fused_gate = fused_gate if fused_gate == "all" else bool(fused_gate)
        # fold_rgb_up: at a level whose same-resolution conv carries the fused ToRGB on the persistent 32 -> 32 kernel or on the
        # weights-resident patch form, that epilogue up-samples the previous level's RGB planes itself (vt_conv2d_rgbup,
        # DESIGN.md 4.1x): no vt_upfirdn2d launch, and the hi-res planes are written once instead of written, read and
        # rewritten.  Bit-identical to `fold_rgb_up=False`, which keeps the two launches for A/B measurements and tests.
        self.fold_rgb_up = bool(fold_rgb_up)
        # style_gate: the style path is skipped ON THE DEVICE when the W+ rows and d_s of a call equal the ones its
        # products were computed from (vt_style_gate: a bitwise compare in the frame's graph, no host sync) -- what the
        # video loop's `s_w.repeat(B,1,1)` (style_transfer.py:176: a new tensor per call, same content) needs; the
        # object-identity cache (cache_styles) never hits there.  Outputs are bit-identical to recomputing.  The
        # drop-in module turns it on; bench.py's `value` does not (it recomputes the style path every step).
        self.style_gate = bool(style_gate)
        # VT_GRAPH_FIRST=1 (default): capture the hipGraph on the first call of a shape; 0 = on the second (one-off shapes
        # then never pay a capture)
        self.graph_first = os.environ.get("VT_GRAPH_FIRST", "1") != "0"
        # up-sampling StyledConvs as conv_transpose2d + LDS blur (vt_conv_desc.up_fir, 9 MACs per input pixel); the polyphase
        # form (36) only when the FIR is not separable (checked in _pack_static)
        self.use_upblur = True
        # per-layer plan overrides {conv_signature(desc): vt_conv_desc.tile_hint}: lets a measured table
        # (tools/plan_sweep.py) pick tile / split-K / kernel family per conv geometry without a rebuild.
        # Like the built-in heuristics the key never contains the batch, so frames stay batch-invariant.
        self.tile_hints: Dict[str, int] = dict(tile_hints or {})
        if not self.tile_hints and os.environ.get("VT_TILE_HINTS"):
            import json
            with open(os.environ["VT_TILE_HINTS"]) as f:
                self.tile_hints = {k: int(v) for k, v in json.load(f).items()}
        self.sd = {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in state_dict.items()}
        self.g = "generator.generator." if self.dual else "generator."
        self.n_down = 0
        while f"encoder.{self.n_down}.0.weight" in self.sd:
            self.n_down += 1
        self.n_fuse = sum(1 for lvl in range(5) if 2 ** (5 + lvl) <= in_size)
        # plans are an LRU (a plan = activations + modulated weights + a hipGraph, ~0.7 GB at 22x256x256): an image-mode
        # caller that feeds many crop sizes would otherwise grow memory without bound.  VT_MAX_PLANS
        # overrides the bound (default 12: three lanes x four shapes).
        import collections
        self._plans: "collections.OrderedDict[tuple, _Plan]" = collections.OrderedDict()
        self.max_plans = max(1, int(os.environ.get("VT_MAX_PLANS", "12")))
        self._shape_seen: Dict[tuple, int] = {}
        self._pack_static()

    # ------------------------------------------------------------------ static weights
    def _pack_static(self):
        sd, T = self.sd, self.dtype
        self.w: Dict[str, torch.Tensor] = {}
        for bi in range(self.n_down):
            for j in (0, 2):
                wsrc = sd[f"encoder.{bi}.{j}.weight"]
                # input channels padded (zero weights) to the 128-byte K-step of the direct-to-LDS / patch kernels:
                # the 32-channel stem output (encoder.0.0 -> encoder.0.2) otherwise drops to the register-staged loader
                # ... except behind a 32-channel stem in bf16: 32 -> 32 and 32 -> 128 are the persistent register-weight
                # kernel's shapes (conv3x3_c32_kernel, 64-byte pixel rows), so neither the stem's input (22 -> 32 channels,
                # zeros) nor its output (32, not 64) is padded to a K-step of zero weights
                cin_dst = self._kpad(wsrc.shape[1]) if j == 2 else None
                if self._stem32(bi):
                    cin_dst = 32
                self.w[f"encoder.{bi}.{j}"] = K.pack_conv_weight(wsrc, cin_dst=cin_dst, out_dtype=T)
        for ii in range(6):
            for nm in ("conv", "conv2"):
                key = f"encoder.{self.n_down}.{ii}.{nm}"
                self.w[key] = K.pack_conv_weight(sd[key + ".weight"], out_dtype=T)
        self.w["enc_rgb"] = K.pack_conv_weight(sd[f"encoder.{self.n_down + 1}.weight"], out_dtype=T)
        if self.dual:
            for ii in range(1, 7):
                for nm in ("conv", "conv2"):
                    w = sd[f"res.{ii}.{nm}.0.weight"]
                    scale = 1.0 / math.sqrt(w.shape[1] * w.shape[2] * w.shape[3])  # EqualConv2d, model.py:101
                    self.w[f"res.{ii}.{nm}"] = K.pack_conv_weight(w, scale=scale, out_dtype=T)
        for fi in range(self.n_fuse):
            if self.dual:
                self.w[f"fusion_out.{fi}.conv"] = K.pack_conv_weight(sd[f"fusion_out.{fi}.conv.weight"], out_dtype=T)
                self.w[f"fusion_out.{fi}.conv2"] = K.pack_conv_weight(sd[f"fusion_out.{fi}.conv2.weight"], out_dtype=T)
            else:
                self.w[f"fusion_out.{fi}"] = K.pack_conv_weight(sd[f"fusion_out.{fi}.weight"], out_dtype=T)
            wsk = sd[f"fusion_skip.{fi}.weight"]  # (3, C+3, 3, 3): cat[skip(3), f_E(*m)]
            c = wsk.shape[1] - 3
            cmap = torch.tensor([0, 1, 2] + [-1] * (SKIP_HDR - 3) + list(range(3, c + 3)), dtype=torch.int32,
                                device=self.device)
            self.w[f"fusion_skip.{fi}"] = K.pack_conv_weight(wsk, cin_dst=c + SKIP_HDR, chan_map=cmap, out_dtype=T)
        # modulated conv weights stay fp32 (cout, cin, k, k); they are re-modulated per style
        self.modw = {}
        for i in range(6, 16):
            self.modw[f"convs.{i}"] = sd[f"{self.g}convs.{i}.conv.weight"][0].contiguous()
        for i in range(3, 8):
            self.modw[f"to_rgbs.{i}"] = sd[f"{self.g}to_rgbs.{i}.conv.weight"][0].contiguous()
            self.w[f"to_rgbs.{i}.bias"] = sd[f"{self.g}to_rgbs.{i}.bias"].reshape(3).contiguous()
        self.fir_up = sd[f"{self.g}convs.6.conv.blur.kernel"].contiguous()
        self.fir_rgb = sd[f"{self.g}to_rgbs.3.upsample.kernel"].contiguous()
        if self.use_upblur:   # the LDS blur is separable: the FIR must be an outer product (make_kernel of a 1-D list)
            k = self.fir_up.detach().float().cpu()
            if not (k.shape == (4, 4) and float(k.sum()) != 0.0 and
                    torch.allclose(torch.outer(k.sum(1), k.sum(0)) / k.sum(), k, rtol=1e-5, atol=1e-7)):
                self.use_upblur = False
        # fragment-stream images of the static 3x3 weights (vt_conv_weight_stream): lets vt_conv2d run the
        # few-pixel / wide-channel layers (the H/8 x W/8 trunk) on the whole-K kernel -- no split-K slabs
        self._wstream: Dict[int, torch.Tensor] = {}
        unit = 8 * (64 if self.h16 else 32)
        for key, wt in self.w.items():
            if wt.ndim == 3 and wt.shape[1] == 9 and wt.shape[2] % unit == 0 and wt.shape[0] % 8 == 0:
                st = K.conv_weight_stream(wt)
                if st is not None:
                    self._wstream[wt.data_ptr()] = st

    def _stem32(self, bi: int) -> bool:
        """Does encoder block `bi` run on 32-channel pixel rows (16-bit, a stem of <= 32 inputs -> 32 -> 32k channels)?"""
        sd = self.sd
        w0, w2 = sd[f"encoder.{bi}.0.weight"], sd[f"encoder.{bi}.2.weight"]
        return (bi == 0 and self.h16 and w0.shape[1] <= 32 and w0.shape[0] == 32 and
                w2.shape[0] % 32 == 0 and w2.shape[0] <= 256)

    def _kpad(self, c: int) -> int:
        """Channel count rounded up to the K-step of the LDS loaders (64 bf16 / fp16, 32 fp32 channels = 128 bytes)."""
        step = 64 if self.h16 else 32
        return (c + step - 1) // step * step

    # ------------------------------------------------------------------ plan helpers
    def _buf(self, plan: _Plan, name: str, shape, dtype=None) -> torch.Tensor:
        t = torch.empty(shape, dtype=dtype or self.dtype, device=self.device)
        plan.bufs[name] = t
        return t

    @staticmethod
    def conv_signature(d) -> str:
        """Geometry key of a conv launch (no batch): 'HxW:cin->cout_total:k3s1d1p1[:nchw]'."""
        return (f"{d.h}x{d.w}:{d.c0 + d.c1}->{d.cout * d.phases}:k{d.kh}s{d.stride}d{d.dil}p{d.phases}"
                + (":nchw" if d.out_layout == OUT_NCHW else "") + (":up" if d.up_fir else ""))

    def _apply_hint(self, d):
        h = self.tile_hints.get(self.conv_signature(d))
        if h:
            d.tile_hint = int(h)
        return d

    def _op_conv(self, ops, plan, ref_macs=None, branch=0, join=False, entry=None, **kw):
        """Append one vt_conv2d launch -- or one of `entry` = (function, arguments after the descriptor, kernel-name suffix,
        extra algorithmic bytes): the forms of include/vtoonify_amd_fusion.h, which run the same descriptor.  The op's info records the kernel instance (tile) and
        its ALGORITHMIC work: flops = 2 x the MACs of the reference contraction it replaces
        (`ref_macs` overrides that for the fused conv_transpose2d+blur form, whose polyphase
        filters do 4x the transposed conv's MACs), bytes = every operand read once + the
        output written once."""
        wt = kw.get("weight")
        if isinstance(wt, torch.Tensor) and wt.data_ptr() in self._wstream:
            kw["weight_stream"] = self._wstream[wt.data_ptr()]
        d = self._apply_hint(K.make_conv_desc(dtype=self.dt_conv, **kw))
        plan.keep.append(d)
        cin = d.c0 + d.c1
        m = d.n * d.out_h * d.out_w
        cout_t = d.cout * d.phases
        macs = m * cout_t * d.kh * d.kw * cin if ref_macs is None else ref_macs
        osz = 4 if d.out_dtype == K.VT_F32 else 2
        # ALGORITHMIC bytes: every operand read once + the output written once -- also when rgb_only skips that write
        # (the op granularity of SURVEY.md 8d; the launch then moves fewer bytes than it is credited with)
        nbytes = (d.n * d.h * d.w * cin * self.esz + cout_t * d.kh * d.kw * cin * self.esz +
                  m * cout_t * osz * (2 if d.resid else 1))
        info = {"name": "conv", "kernel": "conv_igemm", "flops": 2 * macs, "bytes": nbytes, "cin": cin,
                "cout": cout_t, "m": m, "k": d.kh * d.kw * cin, "hw": (d.out_h, d.out_w),
                "sig": self.conv_signature(d)}
        if branch:
            info["branch"] = branch
        if join:
            info["join"] = True
        if entry is not None:
            info["form"] = entry[2]
            info["bytes"] += entry[3]
        plan.convs.append((d, info, ops, len(ops)))
        ops.append((self.lib.vt_conv2d, (C.byref(d),), info) if entry is None else (entry[0], (C.byref(d),) + tuple(entry[1]), info))

    def _conv_kind(self, **kw) -> int:
        """Kernel family vt_conv2d would run this conv on (vt_conv2d_tile KIND; host query, no launch)."""
        wt = kw.get("weight")
        if isinstance(wt, torch.Tensor) and wt.data_ptr() in self._wstream:
            kw["weight_stream"] = self._wstream[wt.data_ptr()]
        d = self._apply_hint(K.make_conv_desc(dtype=self.dt_conv, **kw))
        d.splitk_ws, d.splitk_ws_bytes = 1 << 20, 1 << 40   # "a workspace will exist"
        tile = self.lib.vt_conv2d_tile(C.byref(d))
        return tile // 100000000 if tile >= 0 else -1

    def _rgbup_resident(self, tile: int, n: int, ho: int, wo: int, cout: int) -> bool:
        """Does a same-resolution conv with the fused ToRGB whose plan query returned `tile` run on the weights-resident patch
        form (conv_patch_resident.hpp), the second form vt_conv2d_rgbup carries?  The launch rule of the library, from what
        the query returns and the geometry: a 256 x 64 patch plan of a 64 -> 64 layer without split-K and at least two
        16 x 16 tiles per persistent workgroup (VT_PATCH_PIPE, the library's A/B switch, moves both)."""
        if os.environ.get("VT_PATCH_PIPE", "")[:1] in ("0", "1") or os.environ.get("VT_BATCH_EXACT", "")[:1] == "1":
            return False
        kind, sk, bm, bn = tile // 100000000, (tile // 1000000) % 100, (tile // 1000) % 1000, tile % 1000
        return (kind == 1 and sk <= 1 and bm == 256 and bn == 64 and cout == 64 and
                n * ((ho + 15) // 16) * ((wo + 15) // 16) >= 2 * self._patchw_wgs())

    def _patchw_wgs(self) -> int:
        """Persistent workgroups of the weights-resident form: one per compute unit (VT_PATCHW_WGS: the tests' override)."""
        e = os.environ.get("VT_PATCHW_WGS", "")
        if e.isdigit() and int(e) > 0:
            return int(e)
        if self.device.type == "cuda":
            return torch.cuda.get_device_properties(self.device).multi_processor_count
        return 256

    def _op_linear(self, ops, y, ld_y, x, ld_x, W, b, rows, w_scale=1.0, b_scale=1.0, act=ACT_NONE,
                   slope=0.2, gain=1.0):
        out_dim, in_dim = W.shape
        ops.append((self.lib.vt_linear,
                    (C.c_void_p(K._ptr(y)), ld_y, C.c_void_p(K._ptr(x)), ld_x, C.c_void_p(W.data_ptr()),
                     C.c_void_p(b.data_ptr() if b is not None else 0), rows, in_dim, out_dim,
                     float(w_scale), float(b_scale), act, float(slope), float(gain)), "linear"))

    @staticmethod
    def _info(what):
        if isinstance(what, dict):
            return what
        return {"name": what, "kernel": what, "flops": 0, "bytes": 0}

    def _run(self, ops, stream, plan=None):
        """Issue `ops` in list order on `stream`.  (Graph branches for the style path and the RGB-skip path were measured
        in round 2 -- one frame in flight +1 % / +5 %, three in flight -31 % / -20 %: forked graphs of several lanes collide
        on the graph's internal streams -- and removed in round 4; the ops keep their "branch" / "join" tags as
        documentation of what could run beside the main chain.)"""
        for fn, args, what in ops:
            rc = fn(*args, stream)
            if rc != 0:
                raise _lib.VtError(f"{self._info(what)['name']} failed (code {rc}): "
                                   f"{self.lib.vt_last_error().decode()}")

    # ------------------------------------------------------------------ style path
    def _build_style_ops(self, plan: _Plan, ns: int, has_res: bool):
        """ns = number of distinct style rows prepared (1 when the batch shares a style).

        The ~50 GEMVs of the style path are grouped by dependency level into a handful of
        vt_linear_batch launches, the 15 weight modulations into one vt_modulate_weight_batch."""
        sd, g, ops, lib = self.sd, self.g, plan.style_ops, self.lib
        f32 = torch.float32
        style_in = self._buf(plan, "style_in", (ns, N_LATENT, 512), f32)   # W+ rows
        gate = None
        if self.style_gate:
            style_in.zero_()
            style_new = self._buf(plan, "style_new", (ns, N_LATENT, 512), f32)     # the caller's rows of this call
            gflag = self._buf(plan, "style_gate", (2,), torch.int32)              # [changed, force]
            gflag[0], gflag[1] = 0, 1
            gate = C.c_void_p(gflag.data_ptr())
            ops.append((lib.vt_style_gate, (gate, C.c_void_p(style_in.data_ptr()), C.c_void_p(style_new.data_ptr()),
                                            ns * N_LATENT * 512), "style_gate"))
        ada = self._buf(plan, "adastyles", (ns, N_LATENT, 512), f32)
        ds = self._buf(plan, "d_s", (1,), f32)
        rows = ns * N_LATENT
        levels: List[list] = [[] for _ in range(5)]

        def lin(level, y, ld_y, x, ld_x, W, b, nrows, w_scale=1.0, b_scale=1.0, act=ACT_NONE, slope=0.2,
                gain=1.0):
            it = _lib.LinearItem()
            it.y, it.x, it.W = K._ptr(y), K._ptr(x), W.data_ptr()
            it.b = b.data_ptr() if b is not None else None
            it.ld_y, it.ld_x, it.rows = ld_y, ld_x, nrows
            it.out_dim, it.in_dim = W.shape
            it.act, it.w_scale, it.b_scale, it.slope, it.gain = act, w_scale, b_scale, slope, gain
            levels[level].append(it)

        if self.dual:
            # resstyles = generator.style(style)  (PixelNorm + 2 EqualLinear lr_mul=.01 fused lrelu;
            # model/dualstylegan.py:51-55, model/vtoonify.py:212-220)
            pn = self._buf(plan, "pn", (rows, 512), f32)
            t1 = self._buf(plan, "tc1", (rows, 512), f32)
            res = self._buf(plan, "resstyles", (ns, N_LATENT, 512), f32)
            if gate is not None:
                ops.append((lib.vt_pixel_norm_gated, (C.c_void_p(pn.data_ptr()), C.c_void_p(style_in.data_ptr()), rows, 512,
                                                      gate), "pixel_norm"))
            else:
                ops.append((lib.vt_pixel_norm, (C.c_void_p(pn.data_ptr()), C.c_void_p(style_in.data_ptr()), rows, 512),
                            "pixel_norm"))
            sc = (1.0 / math.sqrt(512)) * 0.01
            lin(0, t1, 512, pn, 512, sd["generator.style.1.weight"], sd["generator.style.1.bias"],
                rows, sc, 0.01, ACT_LRELU, 0.2, SQRT2)
            lin(1, res, 512, t1, 512, sd["generator.style.2.weight"], sd["generator.style.2.bias"],
                rows, sc, 0.01, ACT_LRELU, 0.2, SQRT2)
            # adastyles[:, i] = generator.res[i](adastyles[:, i]), i = 7..17 (vtoonify.py:221-224);
            # rows 0..6 are never read downstream (latent rows 7..17 feed the 15 synthesis convs)
            for i in range(7, N_LATENT):
                lin(0, ada.data_ptr() + i * 512 * 4, N_LATENT * 512, style_in.data_ptr() + i * 512 * 4,
                    N_LATENT * 512, sd[f"generator.res.{i}.weight"], sd[f"generator.res.{i}.bias"], ns,
                    1.0 / math.sqrt(512), 1.0)
        else:
            ops.append((self._copy_op, (ada, style_in), "copy"))

        # modulation vectors + modulated weights of the 15 synthesis convs (model.py:259-267)
        plan.modw = {}
        mods = []
        for lvl in range(5):
            for name, lat, demod, up in ((f"convs.{6 + 2 * lvl}", 7 + 2 * lvl, True, True),
                                         (f"convs.{7 + 2 * lvl}", 8 + 2 * lvl, True, False),
                                         (f"to_rgbs.{3 + lvl}", 9 + 2 * lvl, False, False)):
                w = self.modw[name]
                cout, cin, k, _ = w.shape
                s = self._buf(plan, f"s.{name}", (ns, cin), f32)
                lin(1, s, cin, ada.data_ptr() + lat * 512 * 4, N_LATENT * 512,
                    sd[f"{g}{name}.conv.modulation.weight"], sd[f"{g}{name}.conv.modulation.bias"],
                    ns, 1.0 / math.sqrt(512), 1.0)
                phases = 4 if (up and not self.use_upblur) else 1
                taps = 9 if up else k * k
                wm = self._buf(plan, f"wm.{name}", (ns, phases * cout, taps, cin))
                plan.modw[name] = wm
                for b in range(ns):
                    it = _lib.ModulateItem()
                    it.out = wm.data_ptr() + b * phases * cout * taps * cin * self.esz
                    it.weight, it.s = w.data_ptr(), s.data_ptr() + b * cin * 4
                    it.fir = self.fir_up.data_ptr() if (up and not self.use_upblur) else None
                    it.cout, it.cin, it.k, it.demodulate = cout, cin, k, int(demod)
                    it.scale = 1.0 / math.sqrt(cin * k * k)
                    mods.append(it)
        if self.dual:
            if has_res:
                # AdaIN gamma/beta of the 6 ModRes blocks (dualstylegan.py:16-18), rows resstyles[:, ii+1]
                for ii in range(1, 7):
                    for nm in ("norm", "norm2"):
                        Wl = sd[f"res.{ii}.{nm}.style.weight"]
                        gb = self._buf(plan, f"gb.res.{ii}.{nm}", (ns, Wl.shape[0]), f32)
                        lin(2, gb, Wl.shape[0], plan.bufs["resstyles"].data_ptr() + ii * 512 * 4,
                            N_LATENT * 512, Wl, sd[f"res.{ii}.{nm}.style.bias"], ns)
            # Fusion: label = MLP(d_s) (vtoonify.py:114-124), then AdaIN linear(label)
            # (every row reads the one style degree: row stride 0 -- no broadcast copy)
            for fi in range(self.n_fuse):
                p = f"fusion_out.{fi}."
                l0 = self._buf(plan, f"lab0.{fi}", (ns, 64), f32)
                l1 = self._buf(plan, f"lab1.{fi}", (ns, 128), f32)
                lin(0, l0, 64, ds, 0, sd[p + "linear.0.weight"], sd[p + "linear.0.bias"], ns,
                    1.0, 1.0, ACT_LRELU, 0.2, 1.0)
                lin(1, l1, 128, l0, 64, sd[p + "linear.2.weight"], sd[p + "linear.2.bias"], ns,
                    1.0, 1.0, ACT_LRELU, 0.2, 1.0)
                Wl = sd[p + "norm.style.weight"]
                gb = self._buf(plan, f"gb.fus.{fi}", (ns, Wl.shape[0]), f32)
                lin(2, gb, Wl.shape[0], l1, 128, Wl, sd[p + "norm.style.bias"], ns)
        else:
            # toonify: the modulation linears read `ada` straight after the copy
            pass
        # level 1 of the toonify backbone has no level-0 producers except the copy: still ordered
        for lv in levels:
            if not lv:
                continue
            arr = (_lib.LinearItem * len(lv))(*lv)
            plan.keep.append(arr)
            linfo = {"name": "linear", "kernel": "linear_batch", "flops": 0, "bytes": 0}
            if gate is not None:
                ops.append((lib.vt_linear_batch_gated, (arr, len(lv), gate), linfo))
            else:
                ops.append((lib.vt_linear_batch, (arr, len(lv)), linfo))
        marr = (_lib.ModulateItem * len(mods))(*mods)
        plan.keep.append(marr)
        minfo = {"name": "modulate", "kernel": "modulate_batch", "flops": 0,
                 "bytes": sum(m.cout * m.cin * m.k * m.k * (4 + self.esz * (4 if m.fir else 1)) for m in mods)}
        if gate is not None:
            ops.append((lib.vt_modulate_weight_batch_gated, (marr, len(mods), self.dt, gate), minfo))
        else:
            ops.append((lib.vt_modulate_weight_batch, (marr, len(mods), self.dt), minfo))

    # tiny torch-side helpers used as plan ops (device-to-device copies; plumbing)
    @staticmethod
    def _copy_op(dst, src, stream):
        dst.copy_(src)
        return 0

    @staticmethod
    def _fill_rows_op(dst, src, stream):
        dst.copy_(src.expand_as(dst))
        return 0

    # ------------------------------------------------------------------ frame path
    def _build_plan(self, B: int, H: int, W: int, shared: bool, has_res: bool) -> _Plan:
        sd, g, lib, dt = self.sd, self.g, self.lib, self.dt
        plan = _Plan()
        ns = 1 if shared else B
        self._build_style_ops(plan, ns, has_res)
        f32 = torch.float32
        ops = plan.enc_ops
        ds = plan.bufs["d_s"]

        # ---- content encoder (model/vtoonify.py:160-183, 226-242) -------------------
        cin0 = sd["encoder.0.0.weight"].shape[1]
        cin_p = 32 if self._stem32(0) else _pad8(cin0)
        x_nhwc = self._buf(plan, "x_nhwc", (B, H, W, cin_p))
        if cin_p != _pad8(cin0):
            x_nhwc.zero_()          # the layout change writes pad8(cin0) channels per pixel: the rest stay zero
        plan.cin0 = cin0
        cur, cc, h, w = x_nhwc, cin_p, H, W
        feats = []
        for bi in range(self.n_down):
            stride = 1 if bi == 0 else 2
            for j in (0, 2):
                wt = sd[f"encoder.{bi}.{j}.weight"]
                co = wt.shape[0]
                st = stride if j == 0 else 1
                ho, wo = (h + 2 - 3) // st + 1, (w + 2 - 3) // st + 1
                # the first conv of a block writes into a K-step-padded pixel stride (pad channels stay zero, the next
                # conv's weights for them are zero too): only the 32-channel stem output actually grows (32 -> 64)
                cs = self._kpad(co) if (j == 0 and not self._stem32(bi)) else co
                out = self._buf(plan, f"enc{bi}.{j}", (B, ho, wo, cs))
                if cs != co:
                    out.zero_()
                self._op_conv(ops, plan, src0=cur, c0=cc, ld0=cc, n=B, h=h, w=w, out_h=ho, out_w=wo,
                              weight=self.w[f"encoder.{bi}.{j}"], cout=co, kh=3, kw=3, stride=st, pad=1,
                              bias=sd[f"encoder.{bi}.{j}.bias"], act=ACT_LRELU, slope=0.2, out=out, ld_out=cs)
                cur, cc, h, w = out, cs, ho, wo
            feats.append((cur, cc, h, w))
        feats = feats[::-1]
        # ---- 6 x (VToonifyResBlock [+ AdaResBlock]) at H/8 (vtoonify.py:92-104, 235-239) --
        cf = cc
        tmp = self._buf(plan, "res_tmp", (B, h, w, cf))
        ping = [self._buf(plan, "feat_a", (B, h, w, cf)), self._buf(plan, "feat_b", (B, h, w, cf))]
        hw = h * w
        if self.dual and has_res:
            sc1 = self._buf(plan, "in_scale", (B, cf), f32)
            sh1 = self._buf(plan, "in_shift", (B, cf), f32)
            ws = self._buf(plan, "in_ws", (max(K.instnorm_ws_bytes(B, hw, cf), 16),), torch.uint8)
            nrm_res = self._buf(plan, "nrm_res", (B, h, w, cf))
        feat = cur
        pp = 0
        rk = f"encoder.{self.n_down}"
        # AdaIN of the trunk (dualstylegan.py:6-21,38-45): one vt_instnorm_plane launch per AdaIN for planes of at most 4096
        # pixels (statistics + affine from registers: a 10 us latency chain on a quarter of the CUs, which the other frames in
        # flight fill) between plain convs -- folding it into the whole-K convs (tile records + in-LDS rewrite, round 2) cost
        # +6.5 us in the producer and +17 us in the consumer of a kernel that owns every CU it runs on
        # (profiles/r03_adain_ab.txt).  Larger planes: chunk records from the producing conv's reduce pass + one apply pass.
        plane_adain = self.dual and has_res and hw <= 4096
        for ii in range(6):
            self._op_conv(ops, plan, src0=feat, c0=cf, ld0=cf, n=B, h=h, w=w, out_h=h, out_w=w,
                          weight=self.w[f"{rk}.{ii}.conv"], cout=cf, kh=3, kw=3, pad=1,
                          bias=sd[f"{rk}.{ii}.conv.bias"], act=ACT_LRELU, out=tmp, ld_out=cf)
            nxt = ping[pp]; pp ^= 1
            self._op_conv(ops, plan, src0=tmp, c0=cf, ld0=cf, n=B, h=h, w=w, out_h=h, out_w=w,
                          weight=self.w[f"{rk}.{ii}.conv2"], cout=cf, kh=3, kw=3, pad=1,
                          bias=sd[f"{rk}.{ii}.conv2.bias"], act=ACT_LRELU, alpha=1 / SQRT2, beta=1 / SQRT2,
                          resid=feat, ld_res=cf, out=nxt, ld_out=cf,
                          stats_part=ws if (self.dual and has_res and hw <= 16384 and not plane_adain) else None)
            feat = nxt
            if plane_adain:
                r = ii + 1
                dil = _DIL[r]
                gb1, gb2 = plan.bufs[f"gb.res.{r}.norm"], plan.bufs[f"gb.res.{r}.norm2"]
                ldg = 0 if ns == 1 else gb1.shape[1]

                def _plane(dst, src, gb):
                    ops.append((lib.vt_instnorm_plane,
                                (C.c_void_p(dst.data_ptr()), cf, C.c_void_p(src.data_ptr()), cf, C.c_void_p(0), 0, B, hw, cf,
                                 C.c_void_p(gb.data_ptr()), ldg, dt),
                                {"name": "adain", "kernel": "instnorm_plane", "flops": 0,
                                 "bytes": 2 * B * hw * cf * self.esz}))
                # AdaResBlock (dualstylegan.py:38-45): conv(AdaIN(feat)) -> conv2(AdaIN(.)) * d_s + feat
                _plane(nrm_res, feat, gb1)                      # `feat` itself is the residual below: not in place
                self._op_conv(ops, plan, src0=nrm_res, c0=cf, ld0=cf, n=B, h=h, w=w, out_h=h, out_w=w,
                              weight=self.w[f"res.{r}.conv"], cout=cf, kh=3, kw=3, pad=dil, dil=dil,
                              bias=sd[f"res.{r}.conv.1.bias"], act=ACT_LRELU, gain=SQRT2, out=tmp, ld_out=cf)
                _plane(tmp, tmp, gb2)                           # in place: nothing else reads the raw tensor
                nxt = ping[pp]; pp ^= 1
                self._op_conv(ops, plan, src0=tmp, c0=cf, ld0=cf, n=B, h=h, w=w, out_h=h, out_w=w,
                              weight=self.w[f"res.{r}.conv2"], cout=cf, kh=3, kw=3, pad=dil, dil=dil,
                              bias=sd[f"res.{r}.conv2.1.bias"], act=ACT_LRELU, gain=SQRT2, alpha_dev=ds, beta=1.0,
                              resid=feat, ld_res=cf, out=nxt, ld_out=cf)
                feat = nxt
            elif self.dual and has_res:
                r = ii + 1
                dil = _DIL[r]
                # AdaResBlock (dualstylegan.py:38-45): AdaIN folded into the conv loader
                for nm, src, dst in (("norm", feat, tmp), ("norm2", tmp, None)):
                    gb = plan.bufs[f"gb.res.{r}.{nm}"]
                    # AdaIN as statistics + one fused finalize/apply launch (small tensor), written to
                    # its own buffer so that the conv runs the direct-to-LDS loader; the in-loader
                    # affine (in_scale/in_shift of vt_conv2d) costs more in the MFMA loop than this
                    if hw <= 16384:   # fused finalize+apply for small planes; the chunk records come
                        # from the conv that produced `src` (its split-K reduce pass emits them)
                        ops.append((lib.vt_instnorm_apply_stats,
                                    (C.c_void_p(nrm_res.data_ptr()), cf, C.c_void_p(src.data_ptr()), cf, B, hw, cf,
                                     C.c_void_p(gb.data_ptr()), 0 if ns == 1 else gb.shape[1],
                                     C.c_void_p(ws.data_ptr()), dt),
                                    {"name": "adain", "kernel": "instnorm_apply", "flops": 0,
                                     "bytes": 2 * B * hw * cf * self.esz}))
                    else:   # large planes: separate finalize (parallel tree merge) and apply
                        ops.append((lib.vt_instnorm_stats,
                                    (C.c_void_p(sc1.data_ptr()), C.c_void_p(sh1.data_ptr()), C.c_void_p(src.data_ptr()),
                                     cf, C.c_void_p(0), 0, B, hw, cf, C.c_void_p(gb.data_ptr()),
                                     0 if ns == 1 else gb.shape[1], C.c_void_p(ws.data_ptr()), dt),
                                    {"name": "instnorm", "kernel": "instnorm_stats", "flops": 0,
                                     "bytes": B * hw * cf * self.esz}))
                        ops.append((lib.vt_affine_apply,
                                    (C.c_void_p(nrm_res.data_ptr()), cf, C.c_void_p(src.data_ptr()), cf,
                                     C.c_void_p(0), 0, C.c_void_p(sc1.data_ptr()), C.c_void_p(sh1.data_ptr()),
                                     B, hw, cf, dt),
                                    {"name": "affine", "kernel": "affine_apply", "flops": 0,
                                     "bytes": 2 * B * hw * cf * self.esz}))
                    cn = "conv" if nm == "norm" else "conv2"
                    if dst is not None:
                        self._op_conv(ops, plan, src0=nrm_res, c0=cf, ld0=cf, n=B, h=h, w=w, out_h=h, out_w=w,
                                      weight=self.w[f"res.{r}.{cn}"], cout=cf, kh=3, kw=3, pad=dil, dil=dil,
                                      bias=sd[f"res.{r}.{cn}.1.bias"],
                                      act=ACT_LRELU, gain=SQRT2, out=dst, ld_out=cf,
                                      stats_part=ws if hw <= 16384 else None)
                    else:
                        nxt = ping[pp]; pp ^= 1
                        # out * d_s + skip  (d_s read from device memory: graph-replay safe)
                        self._op_conv(ops, plan, src0=nrm_res, c0=cf, ld0=cf, n=B, h=h, w=w, out_h=h, out_w=w,
                                      weight=self.w[f"res.{r}.{cn}"], cout=cf, kh=3, kw=3, pad=dil, dil=dil,
                                      bias=sd[f"res.{r}.{cn}.1.bias"],
                                      act=ACT_LRELU, gain=SQRT2, alpha_dev=ds, beta=1.0, resid=feat, ld_res=cf,
                                      out=nxt, ld_out=cf)
                        feat = nxt
        plan.feat = (feat, cf, h, w)
        skip = self._buf(plan, "skip_enc", (B, 3, h, w), f32)
        self._op_conv(ops, plan, src0=feat, c0=cf, ld0=cf, n=B, h=h, w=w, out_h=h, out_w=w,
                      weight=self.w["enc_rgb"], cout=3, kh=1, kw=1, bias=sd[f"encoder.{self.n_down + 1}.bias"],
                      out=skip, ld_out=0, out_layout=OUT_NCHW, out_dtype=K.VT_F32, branch=1)
        plan.skip_enc = skip

        # ---- synthesis levels (vtoonify.py:245-272) ------------------------------------
        ops = plan.gen_ops
        out, co = feat, cf
        for lvl in range(5):
            hw = h * w
            if lvl < self.n_fuse:
                f_e, ce, he, we = feats[lvl]
                assert (he, we) == (h, w) and ce == co, "encoder/generator size mismatch (H, W must be multiples of 8)"
                fused = bool(self.fused_gate) and (self.fused_gate == "all" or not self.dual or hw >= 8192)
                hdr = 0 if fused else SKIP_HDR     # channels in front of f_E * m_E in the fusion operand
                # fused, Toonify backbone (no mask): the operand IS f_E
                fem = f_e if (fused and not self.dual) else self._buf(plan, f"fem{lvl}", (B, h, w, co + hdr))
                packed = False
                mask = None
                if self.dual:
                    # Fusion.forward (vtoonify.py:122-128)
                    sc = self._buf(plan, f"fsc{lvl}", (B, 2 * co), f32)
                    sh = self._buf(plan, f"fsh{lvl}", (B, 2 * co), f32)
                    ws = self._buf(plan, f"fws{lvl}", (max(K.instnorm_ws_bytes(B, hw, 2 * co), 16),), torch.uint8)
                    gb = plan.bufs[f"gb.fus.{lvl}"]
                    ops.append((lib.vt_instnorm_stats,
                                (C.c_void_p(sc.data_ptr()), C.c_void_p(sh.data_ptr()), C.c_void_p(out.data_ptr()), co,
                                 C.c_void_p(f_e.data_ptr()), co, B, hw, co, C.c_void_p(gb.data_ptr()),
                                 0 if ns == 1 else gb.shape[1], C.c_void_p(ws.data_ptr()), dt),
                                {"name": "instnorm", "kernel": "instnorm_stats", "flops": 0,
                                 "bytes": 2 * B * hw * co * self.esz}))
                    mask = self._buf(plan, f"mask{lvl}", (B, 1, h, w), f32)
                    mask_kw = dict(n=B, h=h, w=w, out_h=h, out_w=w, weight=self.w[f"fusion_out.{lvl}.conv2"], cout=1,
                                   kh=3, kw=3, pad=1, bias=sd[f"fusion_out.{lvl}.conv2.bias"], act=ACT_RELU_TANH,
                                   out=mask, ld_out=0, out_layout=OUT_NCHW, out_dtype=K.VT_F32)
                    # the mask conv forms cat[f_G, |f_G - f_E|] and applies the AdaIN affine in its loader
                    # (vt_conv_desc.in_absdiff + in_scale / in_shift: bit-identical to vt_affine_apply -> conv, without
                    # the launch and the 2C-channel normalised copy) -- not at the H/8 level: 16 tiles per frame cannot hide
                    # the one-step-in-flight second half of the prologue form's K range (38 us against 7 + 18 for the two
                    # launches).  VT_GATE_LOADER (test hook): 0 = the two launches everywhere, 2 = the loader form everywhere.
                    gate_kw = dict(src0=out, c0=co, ld0=co, src1=f_e, c1=co, ld1=co, in_scale=sc, in_shift=sh, in_absdiff=1)
                    gl = os.environ.get("VT_GATE_LOADER", "1")
                    in_loader = (gl != "0" and (hw >= 4096 or gl == "2") and self._conv_kind(**gate_kw, **mask_kw) == 6)
                    if in_loader and fused:
                        # ... and writes f_E * m_E for the pixels of its tiles (vt_conv2d_gate): no pack pass over f_E
                        self._op_conv(ops, plan, **gate_kw, **mask_kw, join=True,
                                      entry=(lib.vt_conv2d_gate, (C.c_void_p(fem.data_ptr()), co), "+fem", B * hw * co * self.esz))
                        packed = True
                    elif in_loader:
                        self._op_conv(ops, plan, **gate_kw, **mask_kw)
                    else:
                        nrm = self._buf(plan, f"nrm{lvl}", (B, h, w, 2 * co))
                        ops.append((lib.vt_affine_apply,
                                    (C.c_void_p(nrm.data_ptr()), 2 * co, C.c_void_p(out.data_ptr()), co,
                                     C.c_void_p(f_e.data_ptr()), co, C.c_void_p(sc.data_ptr()),
                                     C.c_void_p(sh.data_ptr()), B, hw, co, dt),
                                    {"name": "affine", "kernel": "affine_apply", "flops": 0,
                                     "bytes": 4 * B * hw * co * self.esz}))
                        self._op_conv(ops, plan, src0=nrm, c0=2 * co, ld0=2 * co, **mask_kw)
                    plan.masks.append(mask)
                if fem is not f_e and not packed:
                    # (fused: only behind the two-launch mask conv of the H/8 level -- f_E * m_E without a header, ld_out = C)
                    ops.append((lib.vt_fusion_pack,
                                (C.c_void_p(fem.data_ptr()), co + hdr, C.c_void_p(f_e.data_ptr()), co,
                                 C.c_void_p(mask.data_ptr() if mask is not None else 0), C.c_void_p(skip.data_ptr()),
                                 B, hw, co, dt),
                                {"name": "fusion_pack", "kernel": "fusion_pack", "flops": 0, "join": True,
                                 "bytes": B * hw * (co * self.esz + (co + hdr) * self.esz + (16 if hdr else 4))}))
                fo = self._buf(plan, f"fout{lvl}", (B, h, w, co))
                wkey = f"fusion_out.{lvl}.conv" if self.dual else f"fusion_out.{lvl}"
                self._op_conv(ops, plan, src0=out, c0=co, ld0=co, src1=fem.data_ptr() + hdr * self.esz, c1=co,
                              ld1=co + hdr, n=B, h=h, w=w, out_h=h, out_w=w, weight=self.w[wkey], cout=co, kh=3,
                              kw=3, pad=1, bias=sd[wkey + ".bias"], out=fo, ld_out=co)
                sk2 = self._buf(plan, f"fskip{lvl}", (B, 3, h, w), f32)
                skip_kw = dict(n=B, h=h, w=w, out_h=h, out_w=w, weight=self.w[f"fusion_skip.{lvl}"], cout=3, kh=3, kw=3, pad=1,
                               bias=sd[f"fusion_skip.{lvl}.bias"], out=sk2, ld_out=0, out_layout=OUT_NCHW,
                               out_dtype=K.VT_F32, branch=1)
                if fused:
                    # the skip planes as a second source: [skip(3) | zeros | fem] is the conv's K range, not a tensor
                    self._op_conv(ops, plan, src0=fem, c0=co, ld0=co, **skip_kw,
                                  entry=(lib.vt_conv2d_hdr, (C.c_void_p(skip.data_ptr()), 3, SKIP_HDR), "+hdr", B * hw * 12))
                else:
                    self._op_conv(ops, plan, src0=fem, c0=co + hdr, ld0=co + hdr, **skip_kw)
                out, skip = fo, sk2
            n1, n2, n3 = f"convs.{6 + 2 * lvl}", f"convs.{7 + 2 * lvl}", f"to_rgbs.{3 + lvl}"
            c1o = self.modw[n1].shape[0]
            up = self._buf(plan, f"up{lvl}", (B, 2 * h, 2 * w, c1o))
            o2 = self._buf(plan, f"gout{lvl}", (B, 2 * h, 2 * w, c1o))
            rgb = self._buf(plan, f"rgb{lvl}", (B, 3, 2 * h, 2 * w), f32)
            groups = [(0, B)] if ns == 1 else [(b, 1) for b in range(B)]

            def same_conv(b0, nb):
                """The same-resolution StyledConv of frames b0 .. b0 + nb - 1: (descriptor arguments, ToRGB arguments, tile code of
                the plan query with the ToRGB attached, ToRGB fused?, activation not stored?)"""
                sidx = 0 if ns == 1 else b0
                same_kw = dict(src0=up.data_ptr() + b0 * 4 * hw * c1o * self.esz, c0=c1o, ld0=c1o, n=nb,
                               h=2 * h, w=2 * w, out_h=2 * h, out_w=2 * w, weight=plan.modw[n2][sidx], cout=c1o, kh=3, kw=3, pad=1,
                               bias=sd[f"{g}{n2}.activate.bias"], act=ACT_LRELU, gain=SQRT2,
                               out=o2.data_ptr() + b0 * 4 * hw * c1o * self.esz, ld_out=c1o)
                rgb_ptr = rgb.data_ptr() + b0 * 3 * 4 * hw * 4
                rgb_kw = dict(rgb_weight=plan.modw[n3][sidx], rgb_bias=self.w[f"{n3}.bias"], rgb_resid=rgb_ptr, rgb_out=rgb_ptr)
                # ToRGB (1x1 modulated conv, no demod, + bias + up-sampled skip; model.py:383-392) is
                # fused into the StyledConv's epilogue when one tile holds all its channels
                probe = self._apply_hint(K.make_conv_desc(dtype=self.dt_conv, **same_kw, **rgb_kw))
                probe.splitk_ws, probe.splitk_ws_bytes = 1 << 20, 1 << 40   # "a workspace will exist" (host query only)
                tile = self.lib.vt_conv2d_tile(C.byref(probe))
                fuse_rgb = tile >= 0 and tile % 1000 >= c1o and (tile // 1000000) % 100 <= 1
                # (round 4 un-fused it on the 128-channel patch tiles in bf16, where the fused ToRGB had been sent back to the general
                # epilogue after the wrong-image-row defect; with the cause found -- DESIGN.md 4.1n -- the lean / persistent kernels
                # carry it again.  `fuse_rgb128=False` keeps round 4's two launches for A/B measurements.)
                if fuse_rgb and not self.fuse_rgb128 and self.h16 and tile // 100000000 == 1 and tile % 1000 == 128:
                    fuse_rgb = False
                # the LAST level's activation feeds nothing but its ToRGB: with the fused epilogue on the persistent 32 -> 32
                # kernel it is not stored at all (67 MB per 1024^2 frame; vt_conv_desc.rgb_only)
                rgb_only = fuse_rgb and lvl == 4 and tile // 100000000 == 3
                return same_kw, rgb_kw, tile, fuse_rgb, rgb_only

            # The forms whose ToRGB epilogue up-samples the skip itself (vt_conv2d_rgbup): the persistent 32 -> 32 kernel and the
            # weights-resident patch form.  Decided from the first group's plan: the groups of a level share geometry and batch.
            _, _, tile0, fuse0, _ = same_conv(*groups[0])
            fold_up = (self.fold_rgb_up and fuse0 and self.h16 and
                       (tile0 // 100000000 == 3 or self._rgbup_resident(tile0, groups[0][1], 2 * h, 2 * w, c1o)))
            if not fold_up:
                # skip = Upsample(skip): upfirdn2d up=2 pad=(2,1) (model.py:32-50), fp32 planes
                ops.append((lib.vt_upfirdn2d,
                            (C.c_void_p(rgb.data_ptr()), C.c_void_p(skip.data_ptr()), C.c_void_p(self.fir_rgb.data_ptr()),
                             B * 3, h, w, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1, K.VT_F32),
                            {"name": "upfirdn2d", "kernel": "upfirdn2d_tile<f32,up2>", "flops": 0, "branch": 1,
                             "bytes": B * 3 * hw * 5 * 4}))
            for b0, nb in groups:
                sidx = 0 if ns == 1 else b0
                wm1 = plan.modw[n1][sidx]
                wm3 = plan.modw[n3][sidx]
                # StyledConv(upsample): polyphase 3x3 with 4*Cout filters + pixel shuffle.
                # Algorithmic MACs = the reference's conv_transpose2d (9 per in-pixel) + 4x4 blur
                # (16 per out element), not the 36 per in-pixel the polyphase form spends.
                ref_macs = nb * hw * co * c1o * 9 + nb * 4 * hw * c1o * 16
                if self.use_upblur:   # conv_transpose2d on the matrix cores + the FIR blur out of LDS, one kernel
                    self._op_conv(ops, plan, ref_macs=ref_macs, src0=out.data_ptr() + b0 * hw * co * self.esz, c0=co,
                                  ld0=co, n=nb, h=h, w=w, out_h=2 * h, out_w=2 * w, weight=wm1, cout=c1o, kh=3, kw=3,
                                  up_fir=self.fir_up, bias=sd[f"{g}{n1}.activate.bias"], act=ACT_LRELU, gain=SQRT2,
                                  out=up.data_ptr() + b0 * 4 * hw * c1o * self.esz, ld_out=c1o)
                else:
                    self._op_conv(ops, plan, ref_macs=ref_macs, src0=out.data_ptr() + b0 * hw * co * self.esz, c0=co,
                                  ld0=co, n=nb, h=h, w=w, out_h=h, out_w=w, weight=wm1, cout=c1o, kh=3, kw=3, pad=1,
                                  phases=4, bias=sd[f"{g}{n1}.activate.bias"], act=ACT_LRELU, gain=SQRT2,
                                  out=up.data_ptr() + b0 * 4 * hw * c1o * self.esz, ld_out=c1o)
                same_kw, rgb_kw, tile, fuse_rgb, rgb_only = same_conv(b0, nb)
                rgb_ptr = rgb_kw["rgb_out"]
                if fold_up:
                    # Upsample(skip) in the conv's ToRGB epilogue: the lo-res planes of this group's frames are its source
                    lo_ptr = skip.data_ptr() + b0 * 3 * hw * 4
                    self._op_conv(ops, plan, join=True, **same_kw, **rgb_kw, **({"rgb_only": 1} if rgb_only else {}),
                                  entry=(lib.vt_conv2d_rgbup, (C.c_void_p(lo_ptr), C.c_void_p(self.fir_rgb.data_ptr())), ".up",
                                         nb * 3 * hw * 4))
                    continue
                self._op_conv(ops, plan, join=fuse_rgb, **same_kw, **(rgb_kw if fuse_rgb else {}),
                              **({"rgb_only": 1} if rgb_only else {}))
                if not fuse_rgb:
                    self._op_conv(ops, plan, join=True, src0=o2.data_ptr() + b0 * 4 * hw * c1o * self.esz, c0=c1o, ld0=c1o, n=nb,
                                  h=2 * h, w=2 * w, out_h=2 * h, out_w=2 * w, weight=wm3, cout=3, kh=1, kw=1,
                                  bias=self.w[f"{n3}.bias"], beta=1.0, resid=rgb_ptr, out=rgb_ptr, ld_out=0,
                                  out_layout=OUT_NCHW, out_dtype=K.VT_F32)
            out, co, skip, h, w = o2, c1o, rgb, 2 * h, 2 * w
        plan.image = skip
        self._finalize_convs(plan)
        return plan

    def _finalize_convs(self, plan: _Plan):
        """One split-K workspace shared by every conv of the plan (launches are serial on one
        stream), then name the kernel instance each descriptor runs on."""
        need = {}
        for d, info, _, _ in plan.convs:
            b = int(self.lib.vt_conv2d_ws_bytes(C.byref(d)))
            if b < 0:
                raise _lib.VtError(f"vt_conv2d descriptor rejected: {self.lib.vt_last_error().decode()}")
            br = info.get("branch", 0)
            need[br] = max(need.get(br, 0), b)
        wss = {}
        for br, nb in need.items():   # one workspace per branch (launches of a branch are serial on its stream)
            if nb:  # zero-filled: the head of the workspace holds the split-K arrival counters
                wss[br] = torch.zeros((nb,), dtype=torch.uint8, device=self.device)
                plan.bufs["splitk_ws" if br == 0 else f"splitk_ws{br}"] = wss[br]
        tname = {K.VT_BF16: "bf16", K.VT_F16: "f16"}.get(self.dt, "f32")
        inserts = []
        for d, info, ops, pos in plan.convs:
            ws = wss.get(info.get("branch", 0))
            if ws is not None:
                d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel()
            tile = self.lib.vt_conv2d_tile(C.byref(d))
            if tile < 0:
                raise _lib.VtError(f"vt_conv2d descriptor rejected: {self.lib.vt_last_error().decode()}")
            kind, sk, bm, bn = tile // 100000000, (tile // 1000000) % 100, (tile // 1000) % 1000, tile % 1000
            kname = {0: "conv_igemm_kernel", 1: "conv_patch_kernel", 2: "conv_igemm_glds_kernel",
                     3: "conv3x3_c32_kernel", 4: "conv_fullk_kernel", 5: "conv_upblur_kernel",
                     6: "conv_thin_kernel", 7: "conv_patchs2_kernel", 8: "conv_fullkw_kernel", 9: "conv_upblur_rows_kernel",
                     10: "conv_upflat_kernel"}[kind]
            info["kernel"] = f"{kname}<{tname},{bm}x{bn}>" + info.get("form", "")
            info["splitk"] = sk
            if sk > 1 and self.lib.vt_conv2d_splitk_mode(C.byref(d)) == 2:
                # two-pass split-K as two plan ops (slices, reduce): each is one GPU kernel, so the
                # per-kernel timings of bench.py line up with rocprofv3's kernel names.  (Thin outputs --
                # masks, ToRGB, fusion_skip -- finish inside the slice launch: mode 1, one op.)
                d.splitk_phase = 1
                d2 = _lib.ConvDesc.from_buffer_copy(d)
                d2.splitk_phase = 2
                plan.keep.append(d2)
                m, cout_t = info["m"], info["cout"]
                osz = 4 if d.out_dtype == K.VT_F32 else 2
                rk = "conv_splitk_reduce_stats_kernel" if d.stats_part else "conv_splitk_reduce_kernel"
                rinfo = {"name": "splitk_reduce", "kernel": rk, "flops": 0,
                         "bytes": sk * m * ((cout_t + 7) // 8 * 8) * 4 + m * cout_t * osz}
                if info.get("branch"):
                    rinfo["branch"] = info["branch"]
                inserts.append((ops, pos, (self.lib.vt_conv2d, (C.byref(d2),), rinfo)))
        # insert the reduce ops right after their slice ops (back to front keeps positions valid)
        for ops, pos, op in sorted(inserts, key=lambda t: -t[1]):
            ops.insert(pos + 1, op)

    # ------------------------------------------------------------------ public API
    def _stream(self):
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(0)

    def _rows_equal(self, style: torch.Tensor, owner: Optional[torch.Tensor] = None) -> bool:
        """Do all frames of the batch share one style?  Decided without touching the device when the tensor says
        so itself (one row, or an expand() view: stride 0); otherwise ONE comparison + host sync per distinct
        caller tensor `owner` (same object and version counter; a reference is kept so its address cannot be
        recycled), e.g. the `s_w.repeat(B,1,1)` of style_transfer.py:176 reused for every batch of a video."""
        if style.shape[0] == 1 or style.stride(0) == 0:
            return True
        if owner is not None and getattr(self, "_rows_ref", None) is owner and \
                self._rows_ver == getattr(owner, "_version", 0):
            return self._rows_val
        val = bool((style == style[:1]).all().item())
        self._rows_ref, self._rows_ver, self._rows_val = owner, getattr(owner, "_version", 0), val
        return val

    def _auto_lane(self):
        """Lane for the calling HIP stream: frames issued on different streams must not share plan buffers.  Auto lanes
        live in their own namespace ('s', stream id): they can never collide with the explicit integer lanes of
        VideoToonifier / bench.py (a module call on stream X used to be able to get the plan of slot lane k)."""
        if self.device.type != "cuda":
            return 0
        return ("s", torch.cuda.current_stream(self.device).cuda_stream)

    def map_style(self, z: torch.Tensor) -> torch.Tensor:
        """VToonify.zplus2wplus (model/vtoonify.py:285-286): 8-layer mapping network."""
        sd, g = self.sd, self.g
        shape = z.shape
        x = z.detach().to(self.device, torch.float32).reshape(-1, shape[-1]).contiguous()
        x = K.pixel_norm(x)
        sc = (1.0 / math.sqrt(512)) * 0.01
        for i in range(1, 9):
            x = K.linear(x, sd[f"{g}style.{i}.weight"], sd[f"{g}style.{i}.bias"], sc, 0.01, ACT_LRELU, 0.2, SQRT2)
        return x.reshape(shape)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, style: torch.Tensor, d_s=None, return_mask: bool = False,
                return_feat: bool = False, shared_style: Optional[bool] = None,
                use_graph: Optional[bool] = None, lane: Optional[int] = None, borrow: bool = False) -> torch.Tensor:
        """`lane` selects an independent set of plan buffers (activations, split-K workspace, graph):
        frames issued on different HIP streams must use different lanes, so that two frames of a
        video can be in flight on one GPU (frames are independent).  None = one
        lane per calling stream.  `use_graph` None = hipGraph replay on a GPU (captured on the first
        call of a shape), eager launches under host emulation."""
        if x.device.type != self.device.type or (x.device.type == "cuda" and x.device.index != self.device.index):
            raise _lib.VtError(f"input on {x.device}, engine on {self.device}")
        if use_graph is None:
            use_graph = self.device.type == "cuda"
        if lane is None:
            lane = self._auto_lane()
        B, cin, H, W = x.shape
        if H % 8 or W % 8:
            raise _lib.VtError("H and W must be multiples of 8 (util.py:184-187 crops to //8*8)")
        if self.dual and d_s is None:
            raise TypeError("VToonify-D needs a style degree d_s (model/vtoonify.py:124)")
        d_s = 0.0 if d_s is None else float(d_s)
        style_arg = style
        style = style.detach().to(self.device, torch.float32)
        if style.ndim == 2:  # W space (vtoonify.py:212-215)
            style = style[:, None, :].expand(-1, N_LATENT, -1)
            wspace = True
        else:
            wspace = False
        if style.shape[0] not in (1, B):
            raise _lib.VtError("style batch must be 1 or match the frame batch")
        if shared_style is None:
            shared_style = style.shape[0] == 1 or B == 1 or self._rows_equal(style, style_arg)
        has_res = self.dual and d_s != 0.0  # AdaResBlock early-out (dualstylegan.py:40-41)
        key = (B, H, W, bool(shared_style), has_res) + ((lane,) if lane else ())
        plan = self._plans.get(key)
        if plan is None:
            plan = self._build_plan(B, H, W, bool(shared_style), has_res)
            self._plans[key] = plan
            while len(self._plans) > self.max_plans:   # least recently used plan: its buffers and graph are dropped
                # ... but its last replay may still be running on its lane's stream, and the buffers go back to the caching
                # allocator, which only knows the stream that allocated them: the next plan built on another stream could be
                # handed memory that is still being written.  Evictions are rare: drain the device first.
                if self.device.type == "cuda":
                    torch.cuda.synchronize(self.device)
                self._plans.popitem(last=False)
        else:
            self._plans.move_to_end(key)
        if cin != plan.cin0:
            raise _lib.VtError(f"expected {plan.cin0} input channels, got {cin}")
        # ---- per-call inputs into the plan's static buffers ---------------------------
        srows = style[:1] if shared_style else style
        # the style products (modulated weights, AdaIN gamma/beta) live in the plan's own buffers, so the
        # cache key is per plan: lanes that alternate frame by frame each keep their cache warm.  A hit needs
        # the caller's OWN tensor (same object, same version counter, no dtype/device conversion on the way
        # in -- a converted temporary can reuse a freed address with version 0); the plan keeps a reference,
        # so the address cannot be recycled while it is the key.  Edits through `.data` bypass the version
        # counter: pass a new tensor (or cache_styles=False) for those.
        own = style_arg.device == self.device and style_arg.dtype == torch.float32
        skey = (getattr(style_arg, "_version", 0), wspace, bool(shared_style))
        hit = (self.cache_styles and own and getattr(plan, "style_ref", None) is style_arg and
               getattr(plan, "style_key", None) == skey + (d_s,))
        need_style = not hit
        # the frame enters the plan through ONE layout kernel that reads the caller's tensor where it lies (fp32 / bf16 /
        # fp16 NCHW, contiguous); anything else is first copied into a staging buffer.  (Round 2 always staged: a copy
        # kernel per frame in front of the same layout kernel.)
        xd = x.detach()
        if not (xd.is_contiguous() and xd.dtype in (torch.float32, torch.bfloat16, torch.float16)):
            if "x_in" not in plan.bufs:
                self._buf(plan, "x_in", (B, cin, H, W), torch.float32)
            plan.bufs["x_in"].copy_(xd)
            xd = plan.bufs["x_in"]
        xn = plan.bufs["x_nhwc"]
        _lib.check(self.lib.vt_nchw_to_nhwc(C.c_void_p(xn.data_ptr()), xn.shape[-1], C.c_void_p(xd.data_ptr()), B, cin,
                                            H * W, K.dt_code(xd.dtype), self.dt, self._stream()), "vt_nchw_to_nhwc")
        if need_style and self.style_gate:
            # device-side gate: this call's rows go to `style_new`; the first launch of the style path compares them
            # with the rows its products were computed from and skips the rest when nothing changed.  A new d_s is a
            # host-known change: the "force" word
            if not (own and getattr(plan, "up_ref", None) is style_arg and getattr(plan, "up_key", None) == skey):
                plan.bufs["style_new"].copy_(srows)
                plan.up_ref, plan.up_key = (style_arg, skey) if own else (None, None)
            if getattr(plan, "up_ds", None) != d_s:
                plan.bufs["d_s"].fill_(d_s)
                plan.bufs["style_gate"][1:2].fill_(1)
                plan.up_ds = d_s
        elif need_style:
            # the style rows and the style degree are uploaded only when they CHANGED (same caller tensor + version, same
            # float): the style path below still recomputes everything from them every frame unless cache_styles is on
            if not (own and getattr(plan, "up_ref", None) is style_arg and getattr(plan, "up_key", None) == skey):
                plan.bufs["style_in"].copy_(srows)
                plan.up_ref, plan.up_key = (style_arg, skey) if own else (None, None)
            if getattr(plan, "up_ds", None) != d_s:
                plan.bufs["d_s"].fill_(d_s)
                plan.up_ds = d_s
            cacheable = self.cache_styles and own
            plan.style_ref = style_arg if cacheable else None
            plan.style_key = skey + (d_s,) if cacheable else None
        # By default (VT_GRAPH_FIRST=1) the hipGraph of a (shape, lane) is captured on its FIRST call: a video or a benchmark
        # replays it from the second frame on.  VT_GRAPH_FIRST=0 defers the capture to the second call, so that a one-off crop
        # size runs eager launches and pays no warm-up frame, device sync and capture (ADVICE r2 -- opt-in, for image mode)
        seen = self._shape_seen[key] = self._shape_seen.get(key, 0) + 1
        if len(self._shape_seen) > 4096:
            self._shape_seen.clear()
        if use_graph and self.device.type == "cuda" and not return_feat and (seen > 1 or plan.graphs or self.graph_first):
            self._replay(plan, need_style)
        else:
            self._launch(plan, need_style, not return_feat)
        if return_feat:
            feat, cf, h, w = plan.feat
            f = K.nhwc_to_nchw(feat, cf, B, cf, h, w, self.dtype, torch.float32, self.device, feat)
            return f, plan.skip_enc.clone()
        # `borrow`: hand out the plan's own output buffer (valid until the next call on this lane) instead of a copy --
        # for callers that consume the frame at once (video.py packs it to uint8 on the same stream; bench.py)
        image = plan.image if borrow else plan.image.clone()
        if return_mask and self.dual:
            return image, [m if borrow else m.clone() for m in plan.masks]
        return image

    def _launch(self, plan: _Plan, with_style: bool, with_gen: bool = True):
        """Issue the plan's kernels on the current stream (eager or under graph capture).  The frame is already in
        plan.bufs["x_nhwc"] (forward() converts the caller's tensor in place, outside the graph)."""
        stream = self._stream()
        if with_style:
            self._run(plan.style_ops, stream)
        self._run(plan.enc_ops, stream, plan)
        if with_gen:
            self._run(plan.gen_ops, stream, plan)

    def _replay(self, plan: _Plan, with_style: bool):
        """hipGraph replay of the whole frame: ~140 kernel launches become one graph launch
        (SURVEY.md section 7 step 9).  One graph per (plan, style path on/off); the plan's buffers
        are static, so replay is just `x_in`/`style_in`/`d_s` refreshed + hipGraphLaunch."""
        g = plan.graphs.get(with_style)
        if g is None:
            self._launch(plan, with_style)  # warm-up outside capture (module load, first-use init)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch(plan, with_style)
            plan.graphs[with_style] = g
        g.replay()

    # ------------------------------------------------------------------ measurement hooks
    def plan_for(self, B: int, H: int, W: int, shared_style: bool = True, has_res: bool = True) -> _Plan:
        """The plan of a shape: lane 0's if it exists, else the calling stream's own, else the most recently used."""
        key = (B, H, W, bool(shared_style), bool(has_res and self.dual))
        if key in self._plans:
            return self._plans[key]
        auto = self._auto_lane()
        if auto and key + (auto,) in self._plans:
            return self._plans[key + (auto,)]
        for k in reversed(self._plans):
            if k[:5] == key:
                return self._plans[k]
        raise KeyError(key)

    def frame_ops(self, plan: _Plan, with_style: bool = True):
        """Every launch of one frame, in order, as (fn, args, info) -- for per-kernel timing."""
        return (list(plan.style_ops) if with_style else []) + list(plan.enc_ops) + list(plan.gen_ops)

    def time_ops(self, plan: _Plan, iters: int = 5, with_style: bool = True):
        """Per-launch durations from HIP events recorded on the launch stream around every
        kernel of the frame (the whole frame runs `iters` times; durations are averaged).
        Returns [(info, mean_ms)] in launch order.  GPU only."""
        ops = self.frame_ops(plan, with_style)
        stream = self._stream()
        n = len(ops)
        acc = [0.0] * n
        # Event-to-event durations include the dispatch of the event packets themselves.  An EMPTY event pair
        # costs ~5.6 us on MI355X (self.event_gap_ms, median of 64): two packets; with a kernel between them one
        # of the two overlaps the kernel, so the table reports duration - gap / 2 -- calibrated against
        # rocprofv3's begin->end durations of the same launches (profiles/README.md: 16.1 vs 16.15 us for the
        # dominant kernel).  Raw sums are kept in self.last_raw_ms.  An op that is two launches inside the library
        # is one entry.
        cal = [torch.cuda.Event(enable_timing=True) for _ in range(65)]
        for e in cal:
            e.record()
        torch.cuda.synchronize(self.device)
        gaps = sorted(cal[i].elapsed_time(cal[i + 1]) for i in range(64))
        self.event_gap_ms = gaps[len(gaps) // 2]
        for _ in range(iters):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            self._launch_input_only(plan, stream)
            ev[0].record()
            for i, (fn, args, what) in enumerate(ops):
                rc = fn(*args, stream)
                if rc != 0:
                    raise _lib.VtError(f"{self._info(what)['name']} failed: {self.lib.vt_last_error().decode()}")
                ev[i + 1].record()
            torch.cuda.synchronize(self.device)
            for i in range(n):
                acc[i] += ev[i].elapsed_time(ev[i + 1])
        self.last_raw_ms = [a / iters for a in acc]
        return [(self._info(ops[i][2]), max(acc[i] / iters - 0.5 * self.event_gap_ms, 0.0)) for i in range(n)]

    def _launch_input_only(self, plan: _Plan, stream):
        """time_ops: the plan's x_nhwc still holds the last frame forward() converted -- nothing to do."""
        return

    __call__ = forward
