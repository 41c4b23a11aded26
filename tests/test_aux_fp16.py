"""fp16 compute precision of BiSeNet, pSp and RAFT: the eight glue entry points that gained a VT_F16
instance, the three engines against the reference-made goldens, the module and command-line surface.

Glue kernels, per element.  The shapes are those of the bf16 cases of test_glue_ops.py / test_raft_net.py::
test_glue_kernels plus the ones named in the docstrings below; inputs are rounded to fp16 first and the reference sees
the rounded values.  Bounds are the bf16 cases' with half an fp16 ulp (2^-11 |ref|, floor 2^-25: half_ulp of
test_norm_native_ops.py) in the place of half a bf16 ulp:
  * bit-exact against the torch fp32 formula in the kernel's operation order, rounded once to fp16 (RNE): max-pool, the
    nearest gather with gate / add_vec / add, se_apply, eltwise2, gru_blend;
  * resize_bilinear, upsample_bilinear_add: (4 + 2 in_size) eps of the largest |value| + half an fp16 ulp of the float64
    value;
  * channel_mean writes fp32: 1e-5 of the mean of |x| over the fp16-rounded input, as the fp32 case.

Networks against the goldens.  Two bars per output:
  * the CONDITION: bf16 runs in the same test on the same input and fp16's rel_err is at most a quarter of bf16's on
    every single-pass output (3 more mantissa bits = 8x, halved for terms that are not rounding-dominated).  A store that
    still rounds to bf16 inside an fp16 path fails it.  RAFT's flow after several iterations is chaotic on synthetic
    weights and is only printed;
  * the ABSOLUTE bar: twice the larger of the rel_err measured under host emulation and on the MI355X; both
    measurements stand beside each constant.  Every bar is below the bf16 bar of the same network (4e-2 BiSeNet,
    5e-2 pSp).
Every figure is printed ("[aux_fp16] ...") before it is asserted.
"""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, load_golden, load_keys, psnr, rel_err
from vtoonify_amd import _lib, synth
from vtoonify_amd import kernels as K
from vtoonify_amd.bisenet import BiSeNet, BiSeNetEngine
from vtoonify_amd.psp import GradualStyleEncoder, PspEngine
from vtoonify_amd.raft import RAFT, RaftEngine
from test_glue_ops import (EPS, RESIZE_CASES, P, assert_all_nan, assert_bitwise, assert_close, call, nan_buf, nchw, nhwc,
                           rnd, sync)
from test_norm_native_ops import chunk_px, out_tol

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT16 = _lib.VT_F16


def say(what, **figures):
    print(f"[aux_fp16] {what}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()), flush=True)


# ====================================================================================== the eight entry points in fp16
def test_maxpool2d_fp16(dev):
    """test_glue_ops.test_maxpool2d's cases (k/s/p 3/2/1, 2/1/1, 3/1/0, 5/2/2; 1x1, 2x3, 7x5; c 8, 24, 64) and 3/2/1 on
    7x9 with N = 2: bit-exact, -inf padding, NaN slack kept."""
    g = np.random.default_rng(201)
    cases = [(3, k, s, pad, h, w, c) for k, s, pad in [(3, 2, 1), (2, 1, 1), (3, 1, 0), (5, 2, 2)]
             for h, w in [(1, 1), (2, 3), (7, 5)] for c in (8, 24, 64)]
    cases += [(2, 3, 2, 1, 7, 9, c) for c in (8, 24)]
    for n, k, s, pad, h, w, c in cases:
        if h + 2 * pad < k or w + 2 * pad < k:
            continue
        oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
        for negative in (False, True):
            x = rnd(g, (n, h, w, c), F16)
            if negative:
                x = -(x.abs() + 1).to(F16)
            out = nan_buf(n * oh * ow * c, F16, dev)
            call("vt_maxpool2d", P(out), x.to(dev), n, h, w, c, k, s, pad, DT16, K._stream(out))
            sync(dev)
            ref = nhwc(F.max_pool2d(nchw(x.double()), k, s, pad))
            case = f"n{n} k{k} s{s} p{pad} {h}x{w} c{c} neg={negative}"
            assert_bitwise(out[:n * oh * ow * c].view(n, oh, ow, c), ref, case)
            assert_all_nan(out[n * oh * ow * c:], case)


def test_gate_add_nearest_fp16(dev):
    """The bf16 cases (same size, x2, odd ratios both ways) at c = 16 and the x2 / same-size ones at c = 8 and 24, N = 2,
    with and without add_vec / add: bit-exact against the fp32 formula rounded once to fp16."""
    g = np.random.default_rng(202)
    n = 2
    cases = [(h, w, oh, ow, 16) for h, w, oh, ow in [(4, 6, 4, 6), (3, 4, 6, 8), (5, 7, 8, 3), (7, 5, 3, 8), (4, 5, 4, 10)]]
    cases += [(h, w, oh, ow, c) for c in (8, 24) for h, w, oh, ow in [(3, 5, 3, 5), (3, 5, 6, 10)]]
    for h, w, oh, ow, c in cases:
        res = rnd(g, (n, h, w, c), F16)
        gate = rnd(g, (n, c), F32, 0.5, 1.0)
        av = rnd(g, (n, c))
        add = rnd(g, (n, h, w, c), F16)
        for use_av in (False, True):
            for use_add in (False, True):
                out = nan_buf(n * oh * ow * c, F16, dev)
                call("vt_gate_add_nearest", P(out), res.to(dev), gate.to(dev), av.to(dev) if use_av else None,
                     add.to(dev) if use_add else None, n, h, w, c, oh, ow, DT16, K._stream(out))
                sync(dev)
                t = res.float() * gate[:, None, None, :]
                if use_av:
                    t = t + av[:, None, None, :]
                if use_add:
                    t = t + add.float()
                ref = nhwc(F.interpolate(nchw(t), size=(oh, ow), mode="nearest")).to(F16)
                case = f"{h}x{w}->{oh}x{ow} c{c} add_vec={use_av} add={use_add}"
                assert_bitwise(out[:n * oh * ow * c].view(n, oh, ow, c), ref, case)
                assert_all_nan(out[n * oh * ow * c:], case)


def test_resize_bilinear_fp16(dev):
    """RESIZE_CASES of test_glue_ops.py with c = 3, N = 2, both corner conventions, planar and NHWC (ld 3 and 8: columns
    3..7 keep their sentinel), steps 1 and 2 -- among them BiSeNetEngine's two uses: align_corners 0, x2, mul 2 into NHWC
    ld 8, and align_corners 1 with step 2."""
    g = np.random.default_rng(203)
    n, c = 2, 3
    for h, w, vh, vw, step in RESIZE_CASES:
        x = rnd(g, (n, c, h, w))
        xd = x.to(dev)
        for align in (0, 1):
            full = F.interpolate(x.double(), size=(vh, vw), mode="bilinear", align_corners=bool(align))
            oh, ow = -(-vh // step), -(-vw // step)
            for layout, ld in ((_lib.OUT_NCHW, 0), (_lib.OUT_NHWC, c), (_lib.OUT_NHWC, 8)):
                mul = 1.0 if layout == _lib.OUT_NCHW else (2.0 if (vh, vw) == (2 * h, 2 * w) else 0.75)
                ref = full[:, :, ::step, ::step][:, :, :oh, :ow] * mul
                size = n * c * oh * ow if layout == _lib.OUT_NCHW else n * oh * ow * ld
                out = nan_buf(size, F16, dev)
                call("vt_resize_bilinear", P(out), layout, ld, DT16, P(xd), n, c, h, w, vh, vw, align, step, oh, ow, mul,
                     K._stream(out))
                sync(dev)
                if layout == _lib.OUT_NCHW:
                    got = out[:size].view(n, c, oh, ow)
                else:
                    o = out[:size].view(n, oh, ow, ld)
                    got = nchw(o[..., :c])
                    if ld > c:
                        assert_all_nan(o[..., c:], f"pad channels {h}x{w}->{vh}x{vw}")
                case = f"{h}x{w} -> {vh}x{vw} step {step} align {align} layout {layout} ld {ld} mul {mul}"
                assert_all_nan(out[size:], case)
                slack = (4 + 2 * max(h, w)) * EPS * float(ref.abs().max())
                assert_close(got, ref, out_tol(ref, F16, slack), case)


def test_channel_mean_fp16(dev):
    """The bf16 cases (18 chunks with a partial last one, ld > c, c = 8 / 24 / 40) and hw = 1, one chunk - 1, one chunk + 1."""
    g = np.random.default_rng(204)
    one = chunk_px(64)
    assert one == 64 and chunk_px(one + 1) == one
    for n, hw, c, ld in [(2, 1093, 24, 24), (2, 1093, 24, 32), (1, 37, 8, 16), (3, 200, 40, 40), (2, 1, 8, 8),
                         (2, one - 1, 24, 24), (2, one + 1, 24, 32)]:
        x = rnd(g, (n, hw, ld), F16, 1.5, 0.3)
        mean = nan_buf(n * c, F32, dev)
        part = torch.zeros(K.instnorm_ws_bytes(n, hw, c), dtype=torch.uint8, device=dev)
        call("vt_channel_mean", P(mean), x.to(dev), ld, n, hw, c, P(part), DT16, K._stream(mean))
        sync(dev)
        xs = x[..., :c].double()
        case = f"n{n} hw{hw} c{c} ld{ld}"
        assert_close(mean[:n * c].view(n, c), xs.mean(dim=1), 1e-5 * xs.abs().mean(dim=1) + 1e-30, case)
        assert_all_nan(mean[n * c:], case)


def test_se_apply_fp16(dev):
    """The bf16 cases: sc_stride 1 and 2, c = 8 / 16 / 24, N up to 3, odd sizes; bit-exact."""
    g = np.random.default_rng(205)
    for n, oh, ow, c, sh, sw, s in [(2, 5, 7, 16, 5, 7, 1), (2, 4, 3, 24, 7, 5, 2), (1, 3, 3, 8, 5, 6, 2),
                                    (3, 1, 2, 8, 1, 3, 2), (2, 3, 5, 24, 3, 5, 1)]:
        res = rnd(g, (n, oh, ow, c), F16)
        sc = rnd(g, (n, sh, sw, c), F16)
        gate = torch.sigmoid(rnd(g, (n, c)))
        out = nan_buf(n * oh * ow * c, F16, dev)
        call("vt_se_apply", P(out), res.to(dev), gate.to(dev), sc.to(dev), n, oh, ow, c, sh, sw, s, DT16, K._stream(out))
        sync(dev)
        ref = (res.float() * gate[:, None, None, :] + sc.float()[:, ::s, ::s][:, :oh, :ow]).to(F16)
        case = f"{oh}x{ow} from {sh}x{sw} stride {s} c{c}"
        assert_bitwise(out[:n * oh * ow * c].view(n, oh, ow, c), ref, case)
        assert_all_nan(out[n * oh * ow * c:], case)


def test_upsample_bilinear_add_fp16(dev):
    """The bf16 cases and 2x3 -> 4x6, 3x3 -> 5x7 at c = 8 and 24, N = 2."""
    g = np.random.default_rng(206)
    cases = [(h, w, H, W, 8 if H * W > 1024 else 16)
             for h, w, H, W in [(16, 16, 32, 32), (32, 32, 64, 64), (5, 13, 13, 5), (13, 5, 5, 13), (1, 4, 3, 8), (4, 5, 1, 3)]]
    cases += [(h, w, H, W, c) for c in (8, 24) for h, w, H, W in [(2, 3, 4, 6), (3, 3, 5, 7)]]
    n = 2
    for h, w, H, W, c in cases:
        x = rnd(g, (n, h, w, c), F16)
        y = rnd(g, (n, H, W, c), F16)
        out = nan_buf(n * H * W * c, F16, dev)
        call("vt_upsample_bilinear_add", P(out), x.to(dev), y.to(dev), n, h, w, H, W, c, DT16, K._stream(out))
        sync(dev)
        ref = nhwc(F.interpolate(nchw(x.double()), size=(H, W), mode="bilinear", align_corners=True)) + y.double()
        case = f"{h}x{w} -> {H}x{W} c{c}"
        slack = (4 + 2 * max(h, w)) * EPS * (float(x.abs().max()) + float(y.abs().max()))
        assert_close(out[:n * H * W * c].view(n, H, W, c), ref, out_tol(ref, F16, slack), case)
        assert_all_nan(out[n * H * W * c:], case)


def test_eltwise2_gru_blend_fp16(dev):
    """test_raft_net.test_glue_kernels' shape (30 rows, c = 24, row strides 32 / 24 / 40) and c = 24 with ld = 32 on every
    operand; ops 0..2 and the blend bit-exact, pad columns and the slack keep their sentinel."""
    g = np.random.default_rng(207)
    rows, c = 30, 24
    for ld_o, ld_a, ld_b in ((32, 24, 40), (32, 32, 32)):
        a, b = rnd(g, (rows, ld_a), F16), rnd(g, (rows, ld_b), F16)
        for op in (0, 1, 2):
            out = nan_buf(rows * ld_o, F16, dev)
            call("vt_eltwise2", P(out), ld_o, a.to(dev), ld_a, b.to(dev), ld_b, rows, c, op, DT16, K._stream(out))
            sync(dev)
            af, bf = a[:, :c].float(), b[:, :c].float()
            want = af * bf if op == 0 else (af + bf if op == 1 else torch.relu(af + bf))
            o = out[:rows * ld_o].view(rows, ld_o).cpu()
            assert_bitwise(o[:, :c], want.to(F16), f"eltwise2 op {op} ld {ld_o}/{ld_a}/{ld_b}")
            assert_all_nan(o[:, c:], f"eltwise2 op {op} padding")
            assert_all_nan(out[rows * ld_o:], f"eltwise2 op {op} slack")
    for ld in (32, 40):
        h0 = rnd(g, (rows, c), F16)
        z = torch.from_numpy(g.random((rows, c)).astype(np.float32)).to(F16)
        q = rnd(g, (rows, c), F16)
        h = nan_buf(rows * ld, F16, dev)
        h[:rows * ld].view(rows, ld)[:, :c] = h0.to(dev)
        call("vt_gru_blend", P(h), ld, z.to(dev), q.to(dev), rows, c, DT16, K._stream(h))
        sync(dev)
        zf, hf, qf = z.float(), h0.float(), q.float()
        o = h[:rows * ld].view(rows, ld).cpu()
        assert_bitwise(o[:, :c], ((1.0 - zf) * hf + zf * qf).to(F16), f"gru_blend ld {ld}")
        assert_all_nan(o[:, c:], "gru_blend padding")
        assert_all_nan(h[rows * ld:], "gru_blend slack")


# ================================================================================= networks against the goldens
# Absolute bars = 2 x the larger of the two measurements (rel_err; host emulation / MI355X), rounded up to two digits.
BISENET_BAR = 1.9e-3        # worst of the nine golden outputs (cp8): emulation 9.34e-4, MI355X 8.66e-4   (bf16: 8.4e-3)
PSP_BAR = 3.4e-3            # worst of c1 / c3 / y (c3): emulation 1.683e-3, MI355X 1.553e-3             (bf16: 1.2e-2)
RAFT_BAR = {                # RAFT has no bf16 bar; per stage of the first iteration of case a
    "a.fmap1": 5.0e-3,      # emulation 2.460e-3, MI355X 2.326e-3   (bf16: 1.9e-2)
    "a.cnet": 2.2e-3,       # emulation 9.96e-4,  MI355X 1.067e-3   (bf16: 7.1e-3)
    "a.net1": 8.7e-2,       # emulation 4.316e-2, MI355X 3.816e-2   (bf16: 3.2e-1; the GRU state amplifies on synthetic weights)
    "a.delta1": 6.5e-3,     # emulation 3.244e-3, MI355X 2.972e-3   (bf16: 2.5e-2)
}
BISENET_FULL_BAR = 1.7e-3   # parsing_maps 2x3x256^2 against the oracle, MI355X only: 8.23e-4             (bf16: 7.7e-3)
PSP_FULL_BAR = 1.5e-3       # W+ codes of 1x3x256^2 against the oracle, MI355X only: 7.45e-4              (bf16: 6.1e-3)
BF16_BAR = {"bisenet": 4e-2, "psp": 5e-2}     # test_bisenet.py / test_psp.py


def check_ratio_and_bar(net, errs16, errsbf, bar):
    """errs*: name -> rel_err of every single-pass output in fp16 and in bf16; bar: one number or name -> number."""
    bars = bar if isinstance(bar, dict) else {k: bar for k in errs16}
    for k in errs16:
        say(f"{net} {k}", fp16=errs16[k], bf16=errsbf[k], ratio=errs16[k] / errsbf[k], bar=bars[k])
    say(f"{net} worst", fp16=max(errs16.values()), bf16=max(errsbf.values()))
    for k in errs16:
        assert errs16[k] <= errsbf[k] / 4, f"{net} {k}: fp16 {errs16[k]:.3e} is not a quarter of bf16 {errsbf[k]:.3e}"
        assert errs16[k] < bars[k], f"{net} {k}: fp16 {errs16[k]:.3e} over the bar {bars[k]:.1e}"


def _bisenet_errs(dev, dtype, d):
    sd = synth.synth_state_dict(load_keys("bisenet"), 0)
    eng = BiSeNetEngine({k: v.to(dev) for k, v in sd.items()}, 19, dtype, dev)
    assert eng.dtype == dtype and all(t.dtype == dtype for k, t in eng.w.items() if k.endswith((".c1", "stem", ".out")))
    e = {}
    (y, y16, y32), taps = eng.forward(torch.from_numpy(d["s64__x"]).to(dev), taps=True)
    for k in ("res8", "cp8", "cp16"):
        e["s64." + k] = rel_err(taps[k].cpu().numpy(), d["s64__" + k])
    for k, t in (("y", y), ("y16", y16), ("y32", y32)):
        assert t.dtype == F32
        e["s64." + k] = rel_err(t.cpu().numpy(), d["s64__" + k])
    e["s96x64.y"] = rel_err(eng.forward(torch.from_numpy(d["s96x64__x"]).to(dev))[0].cpu().numpy(), d["s96x64__y"])
    for name in ("frame32", "frame40x24"):
        xp = eng.parsing_maps(torch.from_numpy(d[name + "__x"]).to(dev))
        assert tuple(xp.shape) == d[name + "__xp"].shape and xp.dtype == F32
        e[name + ".xp"] = rel_err(xp.cpu().numpy(), d[name + "__xp"])
    return e


def test_bisenet_golden_fp16(dev):
    d, _ = load_golden("bisenet.npz")
    assert BISENET_BAR < BF16_BAR["bisenet"]
    check_ratio_and_bar("BiSeNet", _bisenet_errs(dev, F16, d), _bisenet_errs(dev, BF16, d), BISENET_BAR)


def _psp_errs(dev, dtype, d):
    sd = synth.synth_state_dict(load_keys("psp"), 0)
    eng = PspEngine({k: v.to(dev) for k, v in sd.items()}, 18, dtype, dev)
    assert eng.dtype == dtype and eng.esz == (4 if dtype == F32 else 2)
    y, taps = eng.forward(torch.from_numpy(d["s32__x"]).to(dev), taps=True)
    assert tuple(y.shape) == (2, 18, 512) and y.dtype == F32
    return {"s32.c1": rel_err(taps[6].cpu().numpy(), d["s32__c1"]), "s32.c3": rel_err(taps[23].cpu().numpy(), d["s32__c3"]),
            "s32.y": rel_err(y.cpu().numpy(), d["s32__y"])}


def test_psp_golden_fp16(dev):
    d, _ = load_golden("psp.npz")
    assert PSP_BAR < BF16_BAR["psp"]
    check_ratio_and_bar("pSp", _psp_errs(dev, F16, d), _psp_errs(dev, BF16, d), PSP_BAR)


def _raft_errs(dev, dtype, d):
    eng = RaftEngine(synth.synth_state_dict(load_keys("raft"), 0), dtype, dev)
    assert eng.dtype == dtype and eng.esz == 2
    eng.keep_taps = True
    im1, im2 = (torch.from_numpy(d[k].astype(np.float32)).to(dev) for k in ("a__image1", "a__image2"))
    lo, ups = eng.forward(im1, im2, iters=int(d["a__cfg"][0]))
    T = eng.taps
    to_nchw = lambda t: t.float().permute(0, 3, 1, 2).cpu().numpy()
    assert T["cnet"].dtype == dtype and T["net1"].dtype == dtype          # the GRU rows are 16-bit ...
    assert T["fmap1"].dtype == F32 and T["corr1"].dtype == F32 and lo.dtype == F32 and ups[0].dtype == F32   # ... the islands fp32
    g = d["a__cnet"]
    want = np.concatenate([np.tanh(g[:, :32]), np.maximum(g[:, 32:], 0)], 1)
    single = {"a.fmap1": rel_err(to_nchw(T["fmap1"])[:, ::4], d["a__fmap1"]), "a.cnet": rel_err(to_nchw(T["cnet"])[:, ::4], want),
              "a.net1": rel_err(to_nchw(T["net1"])[:, ::2], d["a__net1"]),
              "a.delta1": rel_err(T["delta1"].cpu().numpy(), d["a__delta1"])}
    later = {"a.corr1": rel_err(T["corr1"].cpu().numpy()[:, ::9], d["a__corr1"]),
             "a.flow_low": rel_err(lo.cpu().numpy(), d["a__flow_low"]), "a.flow_up": rel_err(ups[0].cpu().numpy(), d["a__flow_up"])}
    return eng, single, later


def test_raft_golden_fp16(dev):
    """Case a stage by stage (ratio and bar on fmap1, cnet, net1, delta1; corr1 and the flows after 3 iterations printed),
    case b end to end (printed, finite, right shapes)."""
    d, _ = load_golden("raft_net.npz")
    eng, s16, l16 = _raft_errs(dev, F16, d)
    _, sbf, lbf = _raft_errs(dev, BF16, d)
    for k in l16:
        say(f"RAFT {k} (reported)", fp16=l16[k], bf16=lbf[k])
    check_ratio_and_bar("RAFT", s16, sbf, RAFT_BAR)
    eng.keep_taps = False
    im1, im2 = (torch.from_numpy(d[k].astype(np.float32)).to(dev) for k in ("b__image1", "b__image2"))
    lo, ups = eng.forward(im1, im2, iters=int(d["b__cfg"][0]))
    assert tuple(lo.shape) == d["b__flow_low"].shape and tuple(ups[-1].shape) == d["b__flow_up"].shape
    assert bool(torch.isfinite(lo).all()) and bool(torch.isfinite(ups[-1]).all())
    say("RAFT b end to end (reported)", flow_low=rel_err(lo.cpu().numpy(), d["b__flow_low"]),
        flow_up=rel_err(ups[-1].cpu().numpy(), d["b__flow_up"]))


# ======================================================================================= module and CLI surface
def _ns(**kw):
    return argparse.Namespace(small=False, alternate_corr=False, **kw)


def test_module_surface_fp16(dev):
    d, _ = load_golden("bisenet.npz")
    m = BiSeNet(n_classes=19, compute_dtype=F16)
    m.load_state_dict(synth.synth_state_dict(load_keys("bisenet"), 0))
    m = m.to(dev).eval()
    assert m.compute_dtype == F16 and m.engine().dtype == F16 and m.engine().dt == _lib.VT_F16
    y = m(torch.from_numpy(d["s64__x"]).to(dev))[0]
    assert rel_err(y.cpu().numpy(), d["s64__y"]) < BISENET_BAR
    e = m.engine()
    m.to(dev)
    assert m._engine is None and m.engine() is not e
    m.load_state_dict(m.state_dict())
    assert m._engine is None

    p = GradualStyleEncoder(50, "ir_se", compute_dtype=F16)
    p.load_state_dict(synth.synth_state_dict(load_keys("psp"), 0))
    p = p.to(dev)
    assert p.compute_dtype == F16 and p.engine().dtype == F16 and p.engine().esz == 2
    assert p.engine().w["in"].dtype == F16
    p.to(dev)
    assert p._engine is None
    p.engine()
    p.load_state_dict(p.state_dict())
    assert p._engine is None


def test_raft_mixed_precision_selects_fp16(dev):
    """RAFT(args): mixed_precision=True is fp16 (the reference's autocast), an explicit compute_dtype wins, and
    mixed_precision=False stays today's fp32 to the bit.  RaftFeatures.nbytes() counts 2-byte GRU rows."""
    sd = synth.synth_state_dict(load_keys("raft"), 0)
    assert RAFT(_ns(mixed_precision=True), compute_dtype=F32).compute_dtype == F32
    assert RAFT(_ns(mixed_precision=False), compute_dtype=F16).compute_dtype == F16
    assert RAFT(None).compute_dtype == F32 and RAFT(_ns()).compute_dtype == F32
    m = RAFT(_ns(mixed_precision=True))
    assert m.compute_dtype == F16
    m.load_state_dict(sd)
    assert m._engine is None
    m = m.to(dev).eval()
    e = m.engine()
    assert e.dtype == F16 and e.esz == 2 and e.w["gru.z1"].dtype == F16
    m.to(dev)
    assert m._engine is None
    m.engine()
    m.load_state_dict(sd)
    assert m._engine is None
    g = torch.Generator().manual_seed(11)
    im1, im2 = (torch.rand(1, 3, 64, 64, generator=g) * 255).to(dev), (torch.rand(1, 3, 64, 64, generator=g) * 255).to(dev)
    lo16, up16 = m(im1, im2, iters=1, test_mode=True)
    assert lo16.dtype == F32 and up16.dtype == F32 and bool(torch.isfinite(up16).all())
    feats = m.engine().encode(im1)
    assert feats.ctx.dtype == F16 and all(q.dtype == F32 for q in feats.pyramid)
    assert feats.nbytes() == 64 * (1360 + 400 * 2)          # s = 64 coarse pixels, e = 2 (ParsingSmoother's formula)
    m32 = RAFT(_ns(mixed_precision=False))
    m32.load_state_dict(sd)
    m32 = m32.to(dev).eval()
    assert m32.engine().dtype == F32
    lo, up = m32(im1, im2, iters=1, test_mode=True)
    lo_e, ups_e = RaftEngine(sd, F32, dev).forward(im1, im2, iters=1)
    assert torch.equal(lo, lo_e) and torch.equal(up, ups_e[-1])
    assert m32.engine().encode(im1).nbytes() == 64 * (1360 + 400 * 4)


def _style_cli():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import style_transfer_amd
    return style_transfer_amd


def test_style_cli_aux_precision(dev, tmp_path):
    from test_style_transfer_cli import _clip
    cli = _style_cli()
    opt = cli.parse([])
    assert opt.aux_precision is None and opt.smooth_precision == "fp32"
    _clip(tmp_path, n=3)

    def run(tag, *extra):
        rep = cli.main(["--content", str(tmp_path / "clip.npy"), "--video", "--intrinsic_code", str(tmp_path / "code.npy"),
                        "--ckpt", "synthetic", "--faceparsing_path", "synthetic", "--backbone", "toonify", "--output_path",
                        str(tmp_path / tag), "--batch_size", "2", "--depth", "2", "--precision", "fp16", *extra], device=dev)
        return rep, np.load(rep["output"])

    rep16, v16 = run("a16", "--aux_precision", "fp16")
    assert rep16["parsing_dtype"] == F16 and v16.shape == (3, 64, 96, 3) and v16.dtype == np.uint8
    rep32, v32 = run("a32", "--aux_precision", "fp32")
    assert rep32["parsing_dtype"] == F32
    diff = np.abs(v16.astype(np.int32) - v32.astype(np.int32))
    say("CLI fp16 frame, parsing fp16 vs fp32", max_levels=float(diff.max()), psnr_db=psnr(v16, v32, 255.0))
    assert int(diff.max()) <= 2 and psnr(v16, v32, 255.0) >= 45.0
    rep0, v0 = run("a0")
    assert rep0["parsing_dtype"] == BF16                      # the default: bf16 beside an fp16 frame
    repbf, vbf = run("abf", "--aux_precision", "bf16")
    assert repbf["parsing_dtype"] == BF16 and v0.tobytes() == vbf.tobytes()


def test_smooth_cli_fp16(dev, tmp_path):
    from test_smooth_cli import _clip
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import smooth_parsing_map_amd as cli
    _clip(tmp_path)
    rep = cli.main(["--video_path", str(tmp_path / "clip.npy"), "--output_path", str(tmp_path / "maps"), "--window_size", "2",
                    "--iters", "2", "--raft_path", "synthetic", "--faceparsing_path", "synthetic", "--frame_order", "rgb",
                    "--precision", "fp16"], device=dev)
    got = np.load(rep["output"])
    assert rep["frames"] == 5 and got.shape == (5, 19, 32, 32) and got.dtype == np.float32 and np.isfinite(got).all()


# ================================================================================================= GPU only
def _gpu():
    _lib.use_library(_lib.DEFAULT_LIB)
    assert not _lib.is_emulation()
    return torch.device("cuda:0")


def _range16(what, tensors):
    """Every 16-bit buffer finite; the largest |value| is printed (DESIGN.md 4.1y "Range")."""
    mx = 0.0
    for name, t in tensors:
        if t.dtype in (F16, BF16) and t.numel():
            assert bool(torch.isfinite(t).all()), f"{what}: {name} is not finite"
            mx = max(mx, float(t.float().abs().max()))
    say(f"{what} range", max_abs=mx, of_fp16_max=mx / 65504.0)
    assert mx > 0.0
    return mx


@pytest.mark.gpu
def test_style_cli_smooth_precision_fp16(tmp_path):
    """--smooth_window with --smooth_precision fp16 is smooth_parsing_map_amd.py --precision fp16 followed by
    --parsing_map_path, byte for byte (GPU only: three CLI runs are too slow for the emulation)."""
    from test_smooth_cli import SMOOTH, _clip, _style_args
    dev = _gpu()
    st = _style_cli()
    import smooth_parsing_map_amd as cli
    _clip(tmp_path)
    rep = cli.main(["--video_path", str(tmp_path / "clip.npy"), "--output_path", str(tmp_path / "maps"), "--window_size", "2",
                    "--iters", "2", "--raft_path", "synthetic", "--faceparsing_path", "synthetic", "--frame_order", "rgb",
                    "--precision", "fp16"], device=dev)
    two = np.load(st.main(_style_args(tmp_path, tmp_path / "o2", ("--parsing_map_path", rep["output"])), device=dev)["output"])
    one = np.load(st.main(_style_args(tmp_path, tmp_path / "o1", SMOOTH + ("--smooth_precision", "fp16")), device=dev)["output"])
    assert one.shape == two.shape == (5, 128, 128, 3) and one.tobytes() == two.tobytes()
    fp32 = np.load(st.main(_style_args(tmp_path, tmp_path / "o0", SMOOTH), device=dev)["output"])
    assert fp32.shape == one.shape          # the default pre-pass (fp32) still runs beside it


@pytest.mark.gpu
def test_bisenet_full_size_fp16():
    from oracle import bisenet_oracle as B, vtoonify_oracle as O
    dev = _gpu()
    sd = synth.synth_state_dict(load_keys("bisenet"), 0)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(3)) * 2 - 1
    old = O.set_backend("torch")
    try:
        ref = B.parsing_maps(synth.to_numpy_sd(sd), x.numpy())
    finally:
        O.set_backend(old)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    eng = BiSeNetEngine(sdd, 19, F16, dev)
    y = eng.parsing_maps(x.to(dev))
    ybf = BiSeNetEngine(sdd, 19, BF16, dev).parsing_maps(x.to(dev))
    assert BISENET_FULL_BAR < BF16_BAR["bisenet"]
    check_ratio_and_bar("BiSeNet 2x3x256^2", {"xp": rel_err(y.cpu().numpy(), ref)}, {"xp": rel_err(ybf.cpu().numpy(), ref)},
                        BISENET_FULL_BAR)
    yg = eng.parsing_maps(x.to(dev), use_graph=True)
    assert torch.equal(yg, eng.parsing_maps(x.to(dev), use_graph=True))
    assert torch.equal(yg, y), "graph replay == eager launches"
    # range at the production size: 4 frames, the net at 512 x 512
    x4 = (torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(dev)
    y4 = eng.parsing_maps(x4)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y4).all())
    _range16("BiSeNet 4x512^2", eng._plans[(4, 256, 256, "maps", 0)]["bufs"].items())


@pytest.mark.gpu
def test_psp_full_size_fp16():
    from oracle import psp_oracle as PO, vtoonify_oracle as O
    dev = _gpu()
    sd = synth.synth_state_dict(load_keys("psp"), 0)
    x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(3)) * 2 - 1
    old = O.set_backend("torch")
    try:
        ref = PO.gradual_style_encoder(synth.to_numpy_sd(sd), x.numpy())
    finally:
        O.set_backend(old)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    eng = PspEngine(sdd, 18, F16, dev)
    y = eng.forward(x.to(dev))
    ybf = PspEngine(sdd, 18, BF16, dev).forward(x.to(dev))
    assert PSP_FULL_BAR < BF16_BAR["psp"]
    check_ratio_and_bar("pSp 1x3x256^2", {"y": rel_err(y.cpu().numpy(), ref)}, {"y": rel_err(ybf.cpu().numpy(), ref)},
                        PSP_FULL_BAR)
    yg = eng.forward(x.to(dev), use_graph=True)
    assert torch.equal(yg, eng.forward(x.to(dev), use_graph=True))
    assert torch.equal(yg, y), "graph replay == eager launches"
    torch.cuda.synchronize()
    _range16("pSp 1x256^2", eng._plans[(1, 256, 256)]["bufs"].items())


@pytest.mark.gpu
def test_raft_full_size_fp16(monkeypatch):
    dev = _gpu()
    m = RAFT(_ns(mixed_precision=True))
    m.load_state_dict(synth.synth_state_dict(load_keys("raft"), 0))
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(9)
    base = F.avg_pool2d(torch.rand(1, 3, 520, 520, generator=g), 5, stride=1, padding=2)
    i1, i2 = (base[:, :, 4 + k:516 + k, 4:516].to(dev) * 255.0 for k in (0, 1))      # one slowly moving 512 x 512 pair
    eng = m.engine()
    eng.keep_bufs = []
    lo, up = m(i1, i2, iters=20, test_mode=True)
    torch.cuda.synchronize()
    bufs, eng.keep_bufs = eng.keep_bufs, None
    assert tuple(up.shape) == (1, 2, 512, 512) and bool(torch.isfinite(up).all()) and bool(torch.isfinite(lo).all())
    _range16("RAFT 512^2 x 20 iterations", [(f"buffer {i} {tuple(t.shape)}", t) for i, t in enumerate(bufs)])
    say("RAFT 512^2 x 20 iterations flow", max_abs_px=float(up.abs().max()))
    del bufs
    monkeypatch.setenv("VT_RAFT_GRAPH", "1")
    for _ in range(3):       # eager, capture + replay, replay
        lo_g, up_g = m(i1, i2, iters=20, test_mode=True)
        assert torch.equal(up_g, up) and torch.equal(lo_g, lo), "graph replay == eager launches"
    assert any(isinstance(v, tuple) for v in eng._graphs.values())
