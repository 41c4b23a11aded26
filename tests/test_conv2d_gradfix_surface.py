"""conv2d_gradfix over the reference's whole surface: per-axis stride / padding / dilation / output_padding and fp16 tensors.

The reference hands per-axis tuples and any float dtype to F.conv2d / F.conv_transpose2d (model/stylegan/op/
conv2d_gradfix.py:95-98, 122-132).  Here a pair whose axes differ runs on the generic implicit-GEMM kernel (horizontal
stride / dilation in the high halves of vt_conv_desc.stride / dil), and fp16 tensors on its fp16 instances
(v_mfma_f32_16x16x32_f16).  Every case: forward, grad_input,
grad_weight, grad_bias (and the R1-style second order) against torch autograd on the CPU -- under host emulation on the
CPU and with -m gpu on the MI355X.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_keys, psnr, rel_err
from vtoonify_amd import _lib, synth
from vtoonify_amd.op import conv2d_gradfix

F32_TOL = 1e-4      # of max|ref| (tests/test_ops.py)
F16_TOL = 2e-3      # of max|ref|: ~4 units of fp16 roundoff
F16_2ND_TOL = 4e-3  # second order in fp16 (measured 4.4e-4 under emulation): it differentiates gradients rounded to fp16


def _ops(transposed, s, p, d, groups, opad):
    if transposed:
        return (lambda x, w, b: conv2d_gradfix.conv_transpose2d(x, w, b, stride=s, padding=p, output_padding=opad,
                                                                groups=groups, dilation=d),
                lambda x, w, b: F.conv_transpose2d(x, w, b, stride=s, padding=p, output_padding=opad, groups=groups,
                                                   dilation=d))
    return (lambda x, w, b: conv2d_gradfix.conv2d(x, w, b, stride=s, padding=p, dilation=d, groups=groups),
            lambda x, w, b: F.conv2d(x, w, b, stride=s, padding=p, dilation=d, groups=groups))


def _operands(transposed, N, Ci, H, W, Co, k, groups, seed):
    g = torch.Generator().manual_seed(seed)
    kh, kw = k
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn((Ci, Co // groups, kh, kw) if transposed else (Co, Ci // groups, kh, kw), generator=g) / 3
    b = torch.randn(Co, generator=g)
    return g, x, w, b


def _case(dev, transposed, N, Ci, H, W, Co, k, s, p, d, groups=1, opad=0, seed=0):
    """fp32, first and second order, against torch autograd of F.conv2d / F.conv_transpose2d in fp32 on the CPU."""
    ours, ref = _ops(transposed, s, p, d, groups, opad)
    g, x0, w0, b0 = _operands(transposed, N, Ci, H, W, Co, k, groups, seed)
    x, w, b = [t.clone().to(dev).requires_grad_(True) for t in (x0, w0, b0)]
    xr, wr, br = [t.clone().requires_grad_(True) for t in (x0, w0, b0)]
    y, yr = ours(x, w, b), ref(xr, wr, br)
    assert y.shape == yr.shape and y.dtype == torch.float32
    go = torch.randn(yr.shape, generator=g)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), go.to(dev), create_graph=True)
    rx, rw, rb = torch.autograd.grad(yr, (xr, wr, br), go, create_graph=True)
    u, v = torch.randn(rx.shape, generator=g), torch.randn(rw.shape, generator=g)
    hx, hw = torch.autograd.grad((gx * u.to(dev)).sum() + (gw * v.to(dev)).sum(), (x, w))   # R1-style second order
    qx, qw = torch.autograd.grad((rx * u).sum() + (rw * v).sum(), (xr, wr))
    pairs = ((y, yr), (gx, rx), (gw, rw), (gb, rb), (hx, qx), (hw, qw))
    return max(rel_err(a.detach().cpu().numpy(), r.detach().numpy()) for a, r in pairs)


def _case_f16(dev, transposed, N, Ci, H, W, Co, k, s, p, d, groups=1, opad=0, seed=0, second=False):
    """fp16 tensors: forward and first-order gradients (and optionally the second order) against the same graph of the
    fp16-rounded operands in float64.  Returns (first-order error, second-order error or None)."""
    ours, ref = _ops(transposed, s, p, d, groups, opad)
    g, x0, w0, b0 = _operands(transposed, N, Ci, H, W, Co, k, groups, seed)
    x0, w0, b0 = (t.half() for t in (x0, w0, b0))
    x, w, b = [t.clone().to(dev).requires_grad_(True) for t in (x0, w0, b0)]
    xr, wr, br = [t.double().requires_grad_(True) for t in (x0, w0, b0)]
    y, yr = ours(x, w, b), ref(xr, wr, br)
    go = torch.randn(yr.shape, generator=g).half()
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), go.to(dev), create_graph=second)
    rx, rw, rb = torch.autograd.grad(yr, (xr, wr, br), go.double(), create_graph=second)
    for t in (y, gx, gw, gb):
        assert t.dtype == torch.float16
    first = max(rel_err(a.detach().cpu().numpy(), r.detach().numpy()) for a, r in ((y, yr), (gx, rx), (gw, rw), (gb, rb)))
    if not second:
        return first, None
    u, v = torch.randn(rx.shape, generator=g).half(), torch.randn(rw.shape, generator=g).half()
    hx, hw = torch.autograd.grad((gx * u.to(dev)).float().sum() + (gw * v.to(dev)).float().sum(), (x, w))
    qx, qw = torch.autograd.grad((rx * u.double()).sum() + (rw * v.double()).sum(), (xr, wr))
    assert hx.dtype == torch.float16 and hw.dtype == torch.float16
    return first, max(rel_err(a.cpu().numpy(), r.numpy()) for a, r in ((hx, qx), (hw, qw)))


# (transposed, N, Ci, H, W, k, stride, padding, dilation, groups, output_padding); every case with a thin (cout < 32: planar
# fp32 out of the kernel) and a wide (cout >= 32, % 8 == 0: NHWC out + the tiled layout change) output
PER_AXIS = [
    (False, 2, 8, 9, 7, (3, 3), (2, 1), (1, 0), 1, 1, 0),
    (False, 2, 8, 7, 10, (3, 3), (1, 2), (0, 2), 1, 1, 0),
    (False, 1, 8, 9, 9, (3, 3), 1, (2, 1), (1, 2), 1, 0),
    (False, 1, 8, 10, 8, (3, 3), 1, 1, (2, 1), 1, 0),
    (False, 2, 8, 6, 7, (1, 3), 1, (0, 1), 1, 1, 0),
    (False, 2, 8, 9, 6, (3, 1), (2, 1), (1, 0), 1, 1, 0),
    (False, 1, 8, 10, 6, (5, 1), 1, (2, 0), 1, 1, 0),
    (False, 1, 8, 7, 11, (3, 5), (1, 2), (1, 2), 1, 1, 0),
    (False, 2, 16, 7, 6, (3, 1), 1, (1, 0), (1, 2), 2, 0),
    (True, 2, 8, 5, 6, (3, 3), (2, 1), (0, 1), 1, 1, (1, 0)),
    (True, 1, 8, 6, 5, (3, 3), 1, (0, 1), (2, 1), 1, 0),
    (True, 1, 8, 5, 5, (3, 3), (2, 1), (1, 0), (2, 1), 1, (1, 0)),
    (True, 2, 8, 6, 5, (1, 3), 1, (0, 1), 1, 1, 0),
    (True, 2, 16, 5, 4, (3, 3), (2, 1), (0, 1), 1, 2, 0),
]


@pytest.mark.parametrize("case", PER_AXIS, ids=[f"c{i}" for i in range(len(PER_AXIS))])
def test_per_axis_geometry_fp32(dev, case):
    tr, n, ci, h, w, k, s, p, d, groups, opad = case
    for co in (6 * groups, 32 * groups):
        e = _case(dev, tr, n, ci, h, w, co, k, s, p, d, groups=groups, opad=opad, seed=len(str(case)) + co)
        assert e < F32_TOL, (case, co, e)


F16_CASES = [   # equal axes: the generic kernel's fp16 instances, both output forms, stride 2, dilation 2, transposed, groups
    (False, 2, 8, 9, 7, (3, 3), 1, 1, 1, 1, 0),
    (False, 1, 16, 10, 9, (3, 3), 2, 1, 1, 1, 0),
    (False, 1, 8, 9, 9, (3, 3), 1, 2, 2, 1, 0),
    (False, 2, 8, 8, 8, (1, 1), 1, 0, 1, 1, 0),
    (True, 2, 8, 5, 4, (3, 3), 2, 0, 1, 1, 0),
    (True, 2, 8, 6, 5, (3, 3), 1, 1, 1, 1, 0),
    (False, 2, 16, 6, 6, (3, 3), 1, 1, 1, 2, 0),
    (False, 1, 64, 6, 5, (3, 3), 1, 1, 1, 1, 0),      # 64 channels: whole fp16 K-steps, the direct-to-LDS loader
    # per-axis
    (False, 2, 8, 9, 7, (3, 1), (2, 1), (1, 0), 1, 1, 0),
    (False, 1, 8, 7, 11, (3, 5), (1, 2), (1, 2), (2, 1), 1, 0),
    (True, 2, 8, 5, 6, (3, 3), (2, 1), (0, 1), (1, 2), 1, (1, 0)),
]


@pytest.mark.parametrize("case", F16_CASES, ids=[f"c{i}" for i in range(len(F16_CASES))])
def test_fp16(dev, case):
    tr, n, ci, h, w, k, s, p, d, groups, opad = case
    for co in (6 * groups, 32 * groups):
        e, _ = _case_f16(dev, tr, n, ci, h, w, co, k, s, p, d, groups=groups, opad=opad, seed=len(str(case)) + co)
        assert e < F16_TOL, (case, co, e)


def test_fp16_second_order(dev):
    for co in (6, 32):
        e1, e2 = _case_f16(dev, False, 2, 8, 9, 7, co, (3, 3), 1, 1, 1, seed=co, second=True)
        assert e1 < F16_TOL and e2 < F16_2ND_TOL, (co, e1, e2)
    e1, e2 = _case_f16(dev, True, 2, 8, 5, 6, 32, (3, 3), (2, 1), (0, 1), 1, opad=(1, 0), seed=3, second=True)
    assert e1 < F16_TOL and e2 < F16_2ND_TOL, (e1, e2)


@pytest.mark.parametrize("transposed, chunk", [(False, 5000), (False, 1000), (True, 40000), (True, 5000)],
                         ids=["images", "rows", "transposed-images", "transposed-rows"])
def test_weight_gradient_chunks_fp16_per_axis(dev, chunk, transposed, monkeypatch):
    """_grad_weight_kernel cut into groups of images (1 image per group in fp32, 2 in fp16 at these chunk sizes) and into
    groups of output rows (1 row / 2 rows), per-axis geometry, fp32 and fp16 (bars: 2e-5 and the fp16 tolerance above,
    against the gradient of the rounded operands in float64)."""
    monkeypatch.setattr(conv2d_gradfix, "_GW_CHUNK_BYTES", chunk)
    n, ci, co, h, w = 3, 8, 16, 9, 7
    s, p, d = (2, 1), (1, 0), (1, 2)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(n, ci, h, w, generator=g)
    if transposed:
        wt = torch.randn(ci, co, 3, 3, generator=g) * 0.1
        ref_fn = lambda a, b: F.conv_transpose2d(a, b, stride=s, padding=p, dilation=d)
        our_fn = lambda a, b: conv2d_gradfix.conv_transpose2d(a, b, stride=s, padding=p, dilation=d)
    else:
        wt = torch.randn(co, ci, 3, 3, generator=g) * 0.1
        ref_fn = lambda a, b: F.conv2d(a, b, stride=s, padding=p, dilation=d)
        our_fn = lambda a, b: conv2d_gradfix.conv2d(a, b, stride=s, padding=p, dilation=d)
    v = torch.randn(ref_fn(x, wt).shape, generator=g)
    for dtype, tol in ((torch.float32, 2e-5), (torch.float16, F16_TOL)):
        xr, wr = x.to(dtype).double().requires_grad_(True), wt.to(dtype).double().requires_grad_(True)
        vq = v.to(dtype).double()
        want, = torch.autograd.grad((ref_fn(xr, wr) * vq).sum(), [wr])
        xq, wq = x.to(dtype).to(dev).requires_grad_(True), wt.to(dtype).to(dev).requires_grad_(True)
        got, = torch.autograd.grad(our_fn(xq, wq), [wq], v.to(dtype).to(dev))
        assert got.dtype == dtype and got.shape == wt.shape
        err = float((got.double().cpu() - want).abs().max() / want.abs().max())
        assert err < tol, (chunk, transposed, dtype, err)


def test_equal_pairs_are_the_int_form(dev):
    """No behaviour change: equal pairs give bitwise the tensor of the int form (fp32 and bf16, conv and transposed)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 9, 9, generator=g)
    w = torch.randn(32, 8, 3, 3, generator=g) / 3
    wt = torch.randn(8, 6, 3, 3, generator=g) / 3
    for dtype in (torch.float32, torch.bfloat16):
        xd, wd, wtd = x.to(dtype).to(dev), w.to(dtype).to(dev), wt.to(dtype).to(dev)
        for ww in (wd, wd[:6].contiguous()):
            a = conv2d_gradfix.conv2d(xd, ww, stride=(1, 1), padding=(1, 1), dilation=(2, 2))
            b = conv2d_gradfix.conv2d(xd, ww, stride=1, padding=1, dilation=2)
            assert torch.equal(a, b)
        a = conv2d_gradfix.conv_transpose2d(xd, wtd, stride=(2, 2), padding=[1, 1], dilation=(1, 1))
        b = conv2d_gradfix.conv_transpose2d(xd, wtd, stride=2, padding=1, dilation=1)
        assert torch.equal(a, b)


def test_geometry_arguments_are_ints_or_pairs(dev):
    x, w = torch.randn(1, 8, 5, 5).to(dev), torch.randn(4, 8, 3, 3).to(dev)
    for bad in ((1, 1, 1), 1.5, "1", None):
        with pytest.raises(ValueError):
            conv2d_gradfix.conv2d(x, w, stride=bad)
    with pytest.raises(ValueError):
        conv2d_gradfix.conv2d(x, w, padding=(1,))
    with pytest.raises(NotImplementedError, match="fp64"):
        conv2d_gradfix.conv2d(x.double(), w.double())


# ------------------------------------------------------------------------------ the reference's eager graph in fp16
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["D", "T"])
def test_eager_graph_fp16_vs_oracle(tag):
    """EagerVToonify over a half-precision state_dict with fp16 frames on the GPU, 256 x 256, against the fp32 oracle: its
    PSNR must beat the bf16 eager graph's on the same inputs by at least 10 dB (3 more mantissa bits)."""
    from oracle import vtoonify_oracle as O   # checker only
    from vtoonify_amd.eager import EagerVToonify
    backbone = {"D": "dualstylegan", "T": "toonify"}[tag]
    _lib.use_library(_lib.DEFAULT_LIB)
    assert not _lib.is_emulation()
    dev = torch.device("cuda:0")
    sd = synth.synth_state_dict(load_keys(tag), 0)
    x, s = synth.synth_frames(1, 256, 256, seed=11), synth.synth_style(seed=12)
    old = O.set_backend("torch")
    try:
        ref = O.vtoonify_forward(synth.to_numpy_sd(sd), x.numpy(), s.numpy(), 0.5, backbone)
    finally:
        O.set_backend(old)
    rng = float(ref.max() - ref.min())
    out = {}
    for dtype in (torch.float16, torch.bfloat16):
        sd_dev = {k: v.to(dev).to(dtype) if v.is_floating_point() else v.to(dev) for k, v in sd.items()}
        with torch.no_grad():
            y = EagerVToonify(sd_dev, backbone, 256).forward(x.to(dev).to(dtype), s.to(dev).to(dtype), 0.5)
        assert y.dtype == dtype and tuple(y.shape) == ref.shape
        y = y.float().cpu().numpy()
        assert np.isfinite(y).all()
        out[dtype] = psnr(y, ref, rng)
    print(f"[parity] eager graph {tag} 256^2 vs fp32 oracle: fp16 PSNR {out[torch.float16]:.2f} dB, "
          f"bf16 PSNR {out[torch.bfloat16]:.2f} dB")
    assert out[torch.float16] >= out[torch.bfloat16] + 10.0, out
