"""Normalisation, native-op and frame I/O kernels one by one, per element, against float64 references.

The third part of the per-kernel suite (test_glue_ops.py: glue and style path; test_ops.py / test_engine_fp16.py: the
convolutions): the InstanceNorm / AdaIN family and vt_fusion_pack (norm_glue.hip), vt_fused_bias_act, the gradients
of upfirdn2d, vt_frame_pack / vt_frame_unpack and the two RAFT glue kernels vt_coords_from_flow / vt_convex_upsample.
Entry points are called through `_lib.lib().vt_*` (through vtoonify_amd.op where the autograd wrapper is under test),
every test runs in host emulation and, with -m gpu, on the MI355X.  References are float64 formulas of the reference
project's operations fed the values AS STORED (rounded to bf16 / fp16 first for the 16-bit cases).  Helpers come from
test_glue_ops.py.  Every output is allocated with slack and filled with NaN (0xA5 for bytes): ld padding, untouched
channels and the slack must keep the sentinel.

Notation: u = 2^-24 (largest relative error of one fp32 rounding), EPS = 2u.  The library and the emulation are built
with -ffp-contract=off, so the fp32 sequences are the ones written in the sources.

InstanceNorm / AdaIN, chunked kernels (vt_instnorm_stats + vt_affine_apply, vt_instnorm_apply[_stats])
    Reference: y = gamma (x - m) r + beta, r = 1 / sqrt(var_biased + 1e-5), per (n, c); `|x - other|` is taken in fp32 as
    both the reference project and the kernels take it (one correctly rounded subtraction of stored values).
    Algorithm as written: chunks of P = clamp(ceil(hw / 256), 64, 4096) pixels; per chunk x0 = first pixel,
    s1 = sum(x - x0), s2 = sum((x - x0)^2) in fp32; mean and M2 = sum_k [s2_k - 2 d_k s1_k + n_k d_k^2] (d_k = mean - x0_k)
    merged in fp64; r, scale = gamma r, shift = beta - scale * mean rounded to fp32; out = fl(fl(x scale) + shift).
      * an fp32 sum of P terms in any order is off by at most (P - 1) u of the sum of absolute values; x - x0 adds u, its
        square 3u: c1 = (P + 1) u for s1, c2 = (P + 3) u for s2.
      * mean: |dm| <= c1 A1,  A1 = mean |x - x0(chunk)|.
      * variance: the merge is exact in the computed sums, so dM2 = hw dm^2 + sum e2_k - 2 sum d_k e1_k, i.e.
        dvar <= c2 A2 + 2 c1 B + (c1 A1)^2,  A2 = mean (x - x0)^2,  B = mean |m - x0(chunk)| |x - x0|.
        None of A1, A2, B contains |mean|: they measure the data against the chunk's first pixel, so the bar does not grow
        with |mean| / std (it does grow when x0 itself is an outlier -- but then the outlier is part of the variance).
      * rho = dvar / (2 (var + 1e-5)) + 1.5 EPS: relative error of scale (roundings of r and of gamma r: 2u; 1e-5f for
        1e-5: < u).
      * the one unavoidable term: mean, scale * mean, shift and x * scale are each rounded to fp32 at the size of
        |gamma r m|: 4u, taken as EPS (|x| + 2 |m|) |gamma| r.
        tol(y)     = |gamma| r (|x - m| rho + c1 A1) + EPS (|gamma| r (|x| + 2 |m|) + |beta| + |y|)
        tol(scale) = |gamma| r rho
        tol(shift) = |gamma| r c1 A1 + |gamma r m| (rho + 2 EPS) + EPS |beta|
      * the mean itself, recovered as -shift / scale from an unstyled launch: c1 A1 + half an fp32 ulp of m + half an
        fp32 ulp of scale * m over scale (the two roundings it went through).  This is the check that sees an fp32 merge.
    THE BAR BITES (test_instnorm_bar_bites, CPU only): at mean 1000 / std 0.01 a naive fp32 E[x^2] - E[x]^2 fails it and
    float64 statistics followed by the same fp32 affine pass it.
vt_instnorm_plane (two-pass fp32 in registers)
    The sum of a plane goes through at most D = 16 (per thread) + 6 (shuffle tree) + 3 (waves) = 25 additions:
    dm <= (D + 2) u mean|x|; the second pass is centred on the computed mean (var' = var + dm^2, exact), its sum of
    non-negative terms is off by (D + 3) u:  rho_p = ((D + 3) u + dm^2 / (var + 1e-5)) / 2 + 3 EPS,
        tol(y) = |gamma| r (|x - m| rho_p + dm) + EPS (|gamma r m| + |beta| + |y|).
    This IS wider than the chunked bar on offset planes (dm grows with |mean|: a plain fp32 mean), legitimately: the
    kernel serves the 32 x 32 trunk, whose planes are not offset.  The naive version fails this bar too.
    By reading, `if (ppt > 16) vpw = 1` cannot be reached (lowering vpw lowers ppt);
    test_instnorm_plane_dispatch_is_total confirms it over hw = 1..4096 and every c % 8 == 0 residue.
Constant planes: variance exactly 0, r = 1 / sqrt(1e-5), finite.  The scale / shift form computes
    fl(fl(c scale) + fl(beta - fl(scale c))): exactly beta when c = 0 and, in the chunked kernels, when beta = 0; otherwise
    beta up to the rounding of |gamma r c| (the unavoidable term above, nothing else: rho = 0 and dm = 0 in the bar).
16-bit outputs: half an ulp of the output type on top.  vt_fusion_pack, and everything in vt_fused_bias_act, are BIT-EXACT
    (one fp32 product / the fp32 sequence add, select-multiply, multiply; 16-bit: that fp32 result rounded once; VT_F64:
    the same sequence in double).  Gradients of fused_leaky_relu: 2 EPS |ref| for x (two products), the bias gradient a
    torch sum of those (count * u of the absolute sum, plus the roundings of its terms); second order 3 EPS.
    Two defects fixed with this test: without a bias the plane form added 0.0f, which lost the sign of x = -0.0 where the
    reference kernel and the flat form keep it; and for fp16 on the device the multiply by `scale` and the conversion were
    fused into v_fma_mixlo_f16 (the exact product rounded straight to fp16, -0 turned into +0) instead of the fp32 result
    rounded once.
upfirdn2d gradients: integer data and dyadic taps make every sum exact, so fp32, bf16, fp16 (one rounding of an exact sum)
    and VT_F64 are BIT-EXACT.  VT_F64 on random data: 4 ulps (2^-52) of the absolute-value sum -- the kernel's fma chain
    cannot be matched by a torch formula.
Frame I/O: BIT-EXACT against the numpy formulas of oracle/frames_oracle.py (div, sub, div / clip, add, mul, truncate).
vt_coords_from_flow: one fp32 addition, u |ref|.  vt_convex_upsample: per term k, a_k = |logit_k - max| enters expf with
    relative error u a_k, expf, the 9-term sums, the division and the product add < 16 EPS:
    tol = sum_k (16 + a_k) EPS |w_k 8 flow_k| + 1e-30.  Logits are scaled by 30 and shifted by 100: one weight saturates, and
    a softmax without the max-subtraction overflows.

Grid-stride passes (GPU only): grid_for of norm_glue.hip through vt_affine_apply and vt_fusion_pack, the 8192-block cap of
fba_flat_kernel, the 65536-block cap of frame_io.hip through the one-pixel form (an odd h * w), and the caps of
vt_coords_from_flow / vt_convex_upsample (the latter needs a 606 MB mask).

Left out on purpose: the convolutions, packers and layout changes (own suites); NaN inputs of vt_frame_unpack (undefined in
the reference); fba_plane_kernel's scalar tail loop with VEC > 1, which no launch can reach (the 16-byte form is chosen only
when step_b % VEC == 0, and then every vector is whole).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vtoonify_amd import _lib
from vtoonify_amd import kernels as K
from vtoonify_amd import op
from test_glue_ops import EPS, SLACK, P, assert_all_nan, assert_bitwise, assert_close, call, nan_buf, rnd, sync

U = EPS / 2
F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DT = {F32: _lib.VT_F32, BF16: _lib.VT_BF16, F16: _lib.VT_F16, F64: _lib.VT_F64}
DTYPES = [F32, BF16, F16]
IN_EPS = 1e-5
UNSUPPORTED = 2      # VT_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------ helpers
def half_ulp(a, dtype):
    """Half an ulp of `dtype` at |a| (float64); 0 for fp32 (the fp32 slack already counts its roundings)."""
    if dtype == F32:
        return torch.zeros_like(a)
    _, e = torch.frexp(a.abs())
    if dtype == BF16:
        return torch.ldexp(torch.ones_like(a), e - 9)
    return torch.ldexp(torch.ones_like(a), (e - 12).clamp(min=-25))


def out_tol(ref, dtype, slack):
    slack = torch.as_tensor(slack, dtype=torch.float64).expand_as(ref)
    return half_ulp(ref.abs() + slack, dtype) + slack


def hulp32(a):
    _, e = torch.frexp(a.abs())
    return torch.ldexp(torch.ones_like(a), e - 25)


def strided(x, ld, dev, junk=640.0):
    """(n, hw, c) -> device tensor (n, hw, ld) whose padding holds a value that would be seen if it were read."""
    buf = torch.full(x.shape[:-1] + (ld,), junk, dtype=x.dtype)
    buf[..., :x.shape[-1]] = x
    return buf.to(dev)


def rc_of(name, *args):
    """Return code of an entry point (for the refusals)."""
    ptrs = [P(a) if isinstance(a, torch.Tensor) else a for a in args]
    return getattr(_lib.lib(), name)(*ptrs)


def chunk_px(hw):
    return min(max((hw + 255) // 256, 64), 4096)


def plane_data(g, kind, n, hw, c, dtype):
    """(n, hw, c) planes of one numerical kind, rounded to dtype."""
    z = g.standard_normal((n, hw, c))
    if kind == "normal":
        v = 1.5 * z + 0.3
    elif kind == "off1000_001":
        v = 1000.0 + 0.01 * z
    elif kind == "off1000_1":
        v = 1000.0 + z
    elif kind == "off100_01":
        v = 100.0 + 0.1 * z
    elif kind == "const":
        v = np.broadcast_to(3.0 + 0.25 * np.arange(c), (n, hw, c)).copy()
    elif kind == "zero":
        v = np.zeros((n, hw, c))
    elif kind == "onepix":
        v = np.broadcast_to(2.0 - 0.5 * np.arange(c), (n, hw, c)).copy()
        v[:, hw // 2] += 1.0
    elif kind == "x0out":
        v = z.copy()
        v[:, ::chunk_px(hw)] = 1e4
    else:
        raise ValueError(kind)
    return torch.from_numpy(v.astype(np.float32)).to(dtype)


def cat_values(x, other):
    """The normalised tensor as stored, float64: x, or cat[x, |x - other|] with the difference taken in fp32."""
    if other is None:
        return x.double()
    return torch.cat([x.double(), (x.float() - other.float()).abs().double()], -1)


def in_stats(v):
    m = v.mean(1)
    var = ((v - m[:, None]) ** 2).mean(1)
    return m, var, 1.0 / torch.sqrt(var + IN_EPS)


def chunked_reference(v, gamma, beta):
    """Float64 AdaIN of v (n, hw, C) and the bars of the module docstring for the chunked kernels."""
    n, hw, _ = v.shape
    m, var, r = in_stats(v)
    cp = chunk_px(hw)
    x0 = v[:, ::cp].repeat_interleave(cp, 1)[:, :hw]
    d = (v - x0).abs()
    A1, A2, B = d.mean(1), (d * d).mean(1), ((m[:, None] - x0).abs() * d).mean(1)
    c1, c2 = (cp + 1) * U, (cp + 3) * U
    dm = c1 * A1
    rho = (c2 * A2 + 2 * c1 * B + dm ** 2) / (2 * (var + IN_EPS)) + 1.5 * EPS
    gr = gamma.abs() * r
    y = gamma[:, None] * (v - m[:, None]) * r[:, None] + beta[:, None]
    tol_y = gr[:, None] * ((v - m[:, None]).abs() * rho[:, None] + dm[:, None]) + \
        EPS * (gr[:, None] * (v.abs() + 2 * m.abs()[:, None]) + beta.abs()[:, None] + y.abs())
    return dict(y=y, tol_y=tol_y, m=m, var=var, r=r, dm=dm, scale=gamma * r, tol_scale=gr * rho,
                shift=beta - gamma * r * m, tol_shift=gr * dm + gr * m.abs() * (rho + 2 * EPS) + EPS * beta.abs())


PLANE_D = 25


def plane_reference(v, gamma, beta):
    """Float64 AdaIN and the bar of vt_instnorm_plane (two-pass fp32)."""
    m, var, r = in_stats(v)
    dm = (PLANE_D + 2) * U * v.abs().mean(1)
    rho = 0.5 * ((PLANE_D + 3) * U + dm ** 2 / (var + IN_EPS)) + 3 * EPS
    gr = gamma.abs() * r
    y = gamma[:, None] * (v - m[:, None]) * r[:, None] + beta[:, None]
    tol = gr[:, None] * ((v - m[:, None]).abs() * rho[:, None] + dm[:, None]) + \
        EPS * ((gr * m.abs())[:, None] + beta.abs()[:, None] + y.abs())
    return y, tol


def style_rows(g, n, ctot, ld_gb):
    """style_gb rows [gamma ctot | beta ctot | junk]; gamma of both signs, away from 0."""
    gb = np.full((n, ld_gb), 555.0, dtype=np.float32)
    gam = g.uniform(0.5, 2.0, (n, ctot)) * np.where(g.random((n, ctot)) < 0.3, -1.0, 1.0)
    gb[:, :ctot] = gam
    gb[:, ctot:2 * ctot] = g.standard_normal((n, ctot))
    return torch.from_numpy(gb)


def gamma_beta(gb, n, ctot):
    if gb is None:
        return torch.ones((n, ctot), dtype=F64), torch.zeros((n, ctot), dtype=F64)
    return gb[:, :ctot].double(), gb[:, ctot:2 * ctot].double()


def ws_buf(n, hw, ctot, dev):
    nbytes = K.instnorm_ws_bytes(n, hw, ctot)
    return torch.full((nbytes + SLACK,), 0xA5, dtype=torch.uint8, device=dev), nbytes


def assert_bytes_kept(buf, start, what):
    assert bool((buf[start:].cpu() == 0xA5).all()), f"{what}: bytes past the end were written"


# ------------------------------------------------------------------------------- chunked InstanceNorm / AdaIN family
def _stats_affine(dev, dtype, x, other, gb, n, hw, c, lds):
    """vt_instnorm_stats + vt_affine_apply on strided buffers -> (scale, shift, out) with the sentinels checked."""
    ld_x, ld_o, ld_out, ld_gb = lds
    ctot = 2 * c if other is not None else c
    xd = strided(x, ld_x, dev)
    od = strided(other, ld_o, dev, junk=-320.0) if other is not None else None
    gbd = gb.to(dev) if gb is not None else None
    scale, shift = nan_buf(n * ctot, F32, dev), nan_buf(n * ctot, F32, dev)
    ws, nbytes = ws_buf(n, hw, ctot, dev)
    call("vt_instnorm_stats", scale, shift, xd, ld_x, od, ld_o, n, hw, c, gbd, ld_gb, ws, DT[dtype], K._stream(xd))
    out = nan_buf(n * hw * ld_out, dtype, dev)
    call("vt_affine_apply", out, ld_out, xd, ld_x, od, ld_o, scale, shift, n, hw, c, DT[dtype], K._stream(xd))
    sync(dev)
    assert_bytes_kept(ws, nbytes, "statistics workspace")
    assert_all_nan(scale[n * ctot:], "scale slack")
    assert_all_nan(shift[n * ctot:], "shift slack")
    o = out[:n * hw * ld_out].view(n, hw, ld_out)
    assert_all_nan(o[..., ctot:], "ld_out padding")
    assert_all_nan(out[n * hw * ld_out:], "out slack")
    return scale[:n * ctot].view(n, ctot), shift[:n * ctot].view(n, ctot), o[..., :ctot]


def _fused_apply(dev, dtype, x, gb, n, hw, c, lds, records=None):
    """vt_instnorm_apply (records None) or vt_instnorm_apply_stats on given records -> out (n, hw, c)."""
    ld_x, _, ld_out, ld_gb = lds
    xd = strided(x, ld_x, dev)
    gbd = gb.to(dev) if gb is not None else None
    out = nan_buf(n * hw * ld_out, dtype, dev)
    if records is None:
        ws, nbytes = ws_buf(n, hw, c, dev)
        call("vt_instnorm_apply", out, ld_out, xd, ld_x, n, hw, c, gbd, ld_gb, ws, DT[dtype], K._stream(xd))
    else:
        ws, nbytes = records
        call("vt_instnorm_apply_stats", out, ld_out, xd, ld_x, n, hw, c, gbd, ld_gb, ws, DT[dtype], K._stream(xd))
    sync(dev)
    assert_bytes_kept(ws, nbytes, "statistics workspace")
    o = out[:n * hw * ld_out].view(n, hw, ld_out)
    assert_all_nan(o[..., c:], "ld_out padding")
    assert_all_nan(out[n * hw * ld_out:], "out slack")
    return o[..., :c]


def _chunked_case(dev, dtype, g, n, hw, c, kind, use_other, use_style):
    vec = 4 if dtype == F32 else 8
    ctot = 2 * c if use_other else c
    lds = (c + vec, c + 2 * vec, ctot + 3 * vec, 2 * ctot + 5)
    x = plane_data(g, kind, n, hw, c, dtype)
    other = (x.float() + rnd(g, (n, hw, c), F32, 0.7)).to(dtype) if use_other else None
    gb = style_rows(g, n, ctot, lds[3]) if use_style else None
    gamma, beta = gamma_beta(gb, n, ctot)
    ref = chunked_reference(cat_values(x, other), gamma, beta)
    case = f"{dtype} n{n} hw{hw} c{c} {kind} other={use_other} style={use_style}"
    scale, shift, out = _stats_affine(dev, dtype, x, other, gb, n, hw, c, lds)
    assert_close(scale, ref["scale"], ref["tol_scale"], case + " scale")
    assert_close(shift, ref["shift"], ref["tol_shift"], case + " shift")
    assert_close(out, ref["y"], out_tol(ref["y"], dtype, ref["tol_y"]), case + " affine_apply")
    if not use_style:      # the mean itself: -shift / scale went through two fp32 roundings only
        got_m = -shift.cpu().double() / scale.cpu().double()
        tol_m = (ref["dm"] + hulp32(ref["m"]) + hulp32(ref["m"] * ref["r"]) / ref["r"]) * (1 + 1e-3) + 1e-30
        assert_close(got_m, ref["m"], tol_m, case + " mean (-shift / scale)")
    # the last image alone: bit for bit the image inside the batch
    s1, h1, o1 = _stats_affine(dev, dtype, x[-1:], None if other is None else other[-1:], None if gb is None else gb[-1:],
                               1, hw, c, lds)
    assert_bitwise(s1, scale[-1:], case + " scale, image alone")
    assert_bitwise(h1, shift[-1:], case + " shift, image alone")
    assert_bitwise(o1, out[-1:], case + " out, image alone")
    if use_other or hw > 16384:
        return
    fused = _fused_apply(dev, dtype, x, gb, n, hw, c, lds)
    assert_close(fused, ref["y"], out_tol(ref["y"], dtype, ref["tol_y"]), case + " instnorm_apply")
    assert_bitwise(_fused_apply(dev, dtype, x[-1:], None if gb is None else gb[-1:], 1, hw, c, lds), fused[-1:],
                   case + " instnorm_apply, image alone")
    # records written by the statistics pass alone: vt_instnorm_apply_stats gives the bits of vt_instnorm_apply
    xd = strided(x, lds[0], dev)
    ws, nbytes = ws_buf(n, hw, c, dev)
    tmp = nan_buf(2 * n * c, F32, dev)
    call("vt_instnorm_stats", tmp, tmp[n * c:], xd, lds[0], None, 0, n, hw, c, None, 0, ws, DT[dtype], K._stream(xd))
    assert_bitwise(_fused_apply(dev, dtype, x, gb, n, hw, c, lds, records=(ws, nbytes)), fused, case + " apply_stats")


def _offset_kinds(dtype):
    return ["off1000_001", "off1000_1"] if dtype == F32 else ["off100_01"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_instnorm_chunked_shapes(dev, dtype):
    """Every plane size and channel count where instnorm_partial_kernel changes its walk, on well-conditioned data."""
    g = np.random.default_rng(101)
    big_c = 1040 if dtype == F32 else 2064           # more than 256 channel vectors: the second pass of the cbase loop
    k = 0
    for hw in (1, 63, 64, 65, 129, 64 * 5 + 1, 2049):
        for c in (16, 48):
            _chunked_case(dev, dtype, g, 3 if hw < 2049 else 2, hw, c, "normal", use_other=k % 2 == 1, use_style=k % 3 != 2)
            k += 1
    _chunked_case(dev, dtype, g, 1, 130, 16, "normal", False, True)
    _chunked_case(dev, dtype, g, 3, 65, big_c, "normal", False, True)
    _chunked_case(dev, dtype, g, 2, 65, big_c, "normal", True, False)      # ctot = 2c through the `other` form
    _chunked_case(dev, dtype, g, 1, 66 * 252 + 1, 16, "normal", True, True)     # hw > 256 * 64: 66-pixel chunks, last of 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_instnorm_chunked_numerics(dev, dtype):
    """Offset planes, a plane constant but for one pixel, and an outlier as every chunk's shift x0: the bar has no
    |mean| / std term beyond the rounding of shift and of the final multiply-add."""
    g = np.random.default_rng(102)
    for kind in _offset_kinds(dtype) + ["onepix", "x0out"]:
        for hw, c, n in ((64 * 7 + 1, 48, 3), (4096, 16, 1)):
            _chunked_case(dev, dtype, g, n, hw, c, kind, use_other=False, use_style=False)
            _chunked_case(dev, dtype, g, n, hw, c, kind, use_other=kind == "onepix", use_style=True)
    # hw > 256 * 64 (76-pixel chunks, 253 of them; the fp64 merge adds 1.9e7 where fp32 has an ulp of 2)
    for kind in _offset_kinds(dtype):
        _chunked_case(dev, dtype, g, 1, 64 * 300 + 1, 16, kind, use_other=False, use_style=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_instnorm_constant_plane(dev, dtype):
    """Variance exactly 0: finite, r = 1 / sqrt(1e-5); exactly beta for a zero plane and for the unstyled chunked kernels
    (beta = 0), beta up to the rounding of |gamma r c| otherwise (module docstring)."""
    g = np.random.default_rng(103)
    for hw, c in ((129, 16), (1, 48), (1024, 32)):
        n = 2
        vec = 4 if dtype == F32 else 8
        lds = (c + vec, c + 2 * vec, c + 3 * vec, 2 * c + 5)
        for kind in ("const", "zero"):
            x = plane_data(g, kind, n, hw, c, dtype)
            for use_style in (False, True):
                gb = style_rows(g, n, c, lds[3]) if use_style else None
                gamma, beta = gamma_beta(gb, n, c)
                want = beta[:, None].expand(n, hw, c)
                tol = EPS * (gamma.abs()[:, None] * x.double().abs() / IN_EPS ** 0.5) * 1.5 + EPS * want.abs()
                case = f"{dtype} hw{hw} c{c} {kind} style={use_style}"
                scale, _, out = _stats_affine(dev, dtype, x, None, gb, n, hw, c, lds)
                assert_close(scale, gamma / IN_EPS ** 0.5, 1.5 * EPS * gamma.abs() / IN_EPS ** 0.5, case + " scale")
                outs = [out, _fused_apply(dev, dtype, x, gb, n, hw, c, lds), _plane(dev, dtype, x, None, gb, n, hw, c, lds)]
                for name, o in zip(("affine_apply", "instnorm_apply", "instnorm_plane"), outs):
                    assert bool(torch.isfinite(o.float()).all()), case + " " + name
                    assert_close(o, want, out_tol(want, dtype, tol), case + " " + name)
                    if kind == "zero" or (not use_style and name != "instnorm_plane"):
                        assert_bitwise(o, want.to(dtype), case + " " + name + " exactly beta")


def test_instnorm_apply_plane_limit(dev):
    """hw = 16384 is the largest plane of the fused form; 16385 is refused with VT_ERR_UNSUPPORTED, nothing written."""
    g = np.random.default_rng(104)
    n, c, dtype = 1, 16, BF16
    _chunked_case(dev, dtype, g, n, 16384, c, "normal", False, True)
    x = torch.zeros((16385, c), dtype=dtype, device=dev)
    out = nan_buf(16385 * c, dtype, dev)
    ws, _ = ws_buf(n, 16385, c, dev)
    for name in ("vt_instnorm_apply", "vt_instnorm_apply_stats"):
        assert rc_of(name, out, c, x, c, n, 16385, c, None, 0, ws, DT[dtype], K._stream(x)) == UNSUPPORTED, name
    sync(dev)
    assert_all_nan(out, "refused launch")


# ------------------------------------------------------------------------------------------------ vt_instnorm_plane
def _plane(dev, dtype, x, other, gb, n, hw, c, lds, in_place=False):
    ld_x, ld_o, ld_out, ld_gb = lds
    ctot = 2 * c if other is not None else c
    xd = strided(x, ld_x, dev)
    od = strided(other, ld_o, dev, junk=-320.0) if other is not None else None
    gbd = gb.to(dev) if gb is not None else None
    if in_place:
        call("vt_instnorm_plane", xd, ld_x, xd, ld_x, None, 0, n, hw, c, gbd, ld_gb, DT[dtype], K._stream(xd))
        sync(dev)
        assert bool((xd[..., c:].float().cpu() == 640.0).all()), "in place: ld padding written"
        return xd[..., :c]
    out = nan_buf(n * hw * ld_out, dtype, dev)
    call("vt_instnorm_plane", out, ld_out, xd, ld_x, od, ld_o, n, hw, c, gbd, ld_gb, DT[dtype], K._stream(xd))
    sync(dev)
    o = out[:n * hw * ld_out].view(n, hw, ld_out)
    assert_all_nan(o[..., ctot:], "ld_out padding")
    assert_all_nan(out[n * hw * ld_out:], "out slack")
    return o[..., :ctot]


def _plane_case(dev, dtype, g, n, hw, c, kind, use_other, use_style):
    vec = 4 if dtype == F32 else 8
    ctot = 2 * c if use_other else c
    lds = (c + vec, c + 2 * vec, ctot + 3 * vec, 2 * ctot + 5)
    x = plane_data(g, kind, n, hw, c, dtype)
    other = (x.float() + rnd(g, (n, hw, c), F32, 0.7)).to(dtype) if use_other else None
    gb = style_rows(g, n, ctot, lds[3]) if use_style else None
    y, tol = plane_reference(cat_values(x, other), *gamma_beta(gb, n, ctot))
    case = f"{dtype} n{n} hw{hw} c{c} {kind} other={use_other} style={use_style}"
    out = _plane(dev, dtype, x, other, gb, n, hw, c, lds)
    assert_close(out, y, out_tol(y, dtype, tol), case)
    one = _plane(dev, dtype, x[-1:], None if other is None else other[-1:], None if gb is None else gb[-1:], 1, hw, c, lds)
    assert_bitwise(one, out[-1:], case + " image alone")
    if not use_other:
        assert_bitwise(_plane(dev, dtype, x, None, gb, n, hw, c, lds, in_place=True), out, case + " in place")


def _plane_dispatch(hw, c, vec):
    """(vpw, ppt) as the host function of vt_instnorm_plane derives them."""
    vpw = 4 if hw <= 1024 else 2 if hw <= 2048 else 1
    while vpw > 1 and c % (vec * vpw) != 0:
        vpw >>= 1
    return vpw, (hw + 256 // vpw - 1) // (256 // vpw)


def test_instnorm_plane_dispatch_is_total():
    """No (hw, c) reaches the `ppt > 16` fallback, and the cases of test_instnorm_plane choose every instance."""
    for vec in (4, 8):
        for hw in range(1, 4097):
            for c in range(8, 72, 8):          # the choice depends on c % (4 * vec) only
                vpw, ppt = _plane_dispatch(hw, c, vec)
                assert 1 <= ppt <= 16, (vec, hw, c, vpw, ppt)
        wide = 4 * vec
        seen = set()
        for hw, c in _plane_shapes(vec, wide):
            vpw, _ = _plane_dispatch(hw, c, vec)
            seen.add((4, 4) if vpw == 4 and hw <= 256 else (16, vpw))        # <PPT, VPW> of VT_PLANE_P
        assert seen == {(4, 4), (16, 4), (16, 2), (16, 1)}, (vec, seen)


def _plane_shapes(vec, wide):
    shapes = [(hw, wide) for hw in (1, 256, 257, 1024, 1025, 2048, 2049, 4096)]
    return shapes + [(hw, c) for c in (8, 24) for hw in (256, 257, 1024)] + [(255, 2 * vec), (1000, 2 * vec), (100, 8)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_instnorm_plane(dev, dtype):
    g = np.random.default_rng(105)
    vec = 4 if dtype == F32 else 8
    for k, (hw, c) in enumerate(_plane_shapes(vec, 4 * vec)):
        n = 3 if hw <= 1025 else 2
        _plane_case(dev, dtype, g, n, hw, c, "normal", use_other=False, use_style=k % 2 == 0)
        _plane_case(dev, dtype, g, n, hw, c, "normal", use_other=True, use_style=k % 2 == 1)
    for kind in _offset_kinds(dtype) + ["onepix", "x0out"]:
        _plane_case(dev, dtype, g, 2, 1024, 4 * vec, kind, use_other=False, use_style=True)
        _plane_case(dev, dtype, g, 2, 257, 8, kind, use_other=kind == "onepix", use_style=False)
    x = torch.zeros((4097, 8), dtype=dtype, device=dev)
    out = nan_buf(4097 * 8, dtype, dev)
    assert rc_of("vt_instnorm_plane", out, 8, x, 8, None, 0, 1, 4097, 8, None, 0, DT[dtype], K._stream(x)) == UNSUPPORTED
    sync(dev)
    assert_all_nan(out, "refused launch")


# --------------------------------------------------------------------------------------------------- the bar bites
def _affine32(x32, mean, var, gamma, beta):
    """The kernels' fp32 affine from given statistics: rstd, scale, shift in fp32, fl(fl(x scale) + shift)."""
    rstd = (1.0 / np.sqrt(np.asarray(var, np.float64) + IN_EPS)).astype(np.float32)
    scale = (gamma * rstd).astype(np.float32)
    shift = (beta - scale * np.asarray(mean).astype(np.float32)).astype(np.float32)
    return (x32 * scale + shift).astype(np.float32)


def test_instnorm_bar_bites():
    """At mean 1000 / std 0.01 a naive fp32 E[x^2] - E[x]^2 fails both bars; float64 statistics with the same fp32 affine
    pass them.  The bars sit between the two without a hand-picked number."""
    g = np.random.default_rng(106)
    n, hw, c = 2, 1024, 16
    x = plane_data(g, "off1000_001", n, hw, c, F32)
    gb = style_rows(g, n, c, 2 * c)
    gamma, beta = gamma_beta(gb, n, c)
    v = x.double()
    x32, g32, b32 = x.numpy(), gb[:, None, :c].numpy(), gb[:, None, c:].numpy()
    m32 = x32.mean(1, keepdims=True, dtype=np.float32)
    naive_var = np.maximum((x32 * x32).mean(1, keepdims=True, dtype=np.float32) - m32 * m32, np.float32(0))
    naive = torch.from_numpy(_affine32(x32, m32, naive_var, g32, b32)).double()
    m64 = x32.astype(np.float64).mean(1, keepdims=True)
    v64 = ((x32.astype(np.float64) - m64) ** 2).mean(1, keepdims=True)
    good = torch.from_numpy(_affine32(x32, m64, v64, g32, b32)).double()
    ref = chunked_reference(v, gamma, beta)
    y_p, tol_p = plane_reference(v, gamma, beta)
    for name, y, tol in (("chunked", ref["y"], ref["tol_y"]), ("plane", y_p, tol_p)):
        assert bool(((good - y).abs() <= tol).all()), name + ": float64 statistics + fp32 affine must pass"
        assert bool(((naive - y).abs() > tol).any()), name + ": the naive fp32 variance must fail"
    assert float((tol_p / ref["tol_y"]).min()) > 1.0      # the plane bar is the wider one here, as derived


# ---------------------------------------------------------------------------------------------------- vt_fusion_pack
def _fusion_pack(dev, dtype, skip, f_e, mask, n, hw, c, hdr, ld_e):
    ld_out = hdr + c
    out = nan_buf(n * hw * ld_out, dtype, dev)
    sk = torch.full((n * 3 * hw + 2 * hw,), 5.0)          # defined values behind the three planes
    sk[:n * 3 * hw] = skip.reshape(-1)
    call("vt_fusion_pack", out, ld_out, strided(f_e, ld_e, dev), ld_e, None if mask is None else mask.to(dev), sk.to(dev),
         n, hw, c, DT[dtype], K._stream(out))
    sync(dev)
    assert_all_nan(out[n * hw * ld_out:], "out slack")
    return out[:n * hw * ld_out].view(n, hw, ld_out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fusion_pack(dev, dtype):
    """[skip(3) | zeros | f_E * m_E], bit-exact: header 8 and 64, with and without mask, ld_e > c."""
    g = np.random.default_rng(107)
    for n, hw, c, hdr in ((3, 37, 16, 8), (3, 20, 24, 64), (1, 1, 8, 8), (2, 65, 64, 64)):
        skip, f_e = rnd(g, (n, 3, hw)), rnd(g, (n, hw, c), dtype)
        for mask in (None, rnd(g, (n, hw), F32, 0.3, 0.5)):
            got = _fusion_pack(dev, dtype, skip, f_e, mask, n, hw, c, hdr, c + 16)
            want = torch.zeros((n, hw, hdr + c))
            want[..., :3] = skip.permute(0, 2, 1)
            want[..., hdr:] = f_e.float() * (1.0 if mask is None else mask[..., None])
            case = f"{dtype} n{n} hw{hw} c{c} header {hdr} mask={mask is not None}"
            assert_bitwise(got, want.to(dtype), case)
            one = _fusion_pack(dev, dtype, skip[-1:], f_e[-1:], None if mask is None else mask[-1:], 1, hw, c, hdr, c + 16)
            assert_bitwise(one, got[-1:], case + " image alone")


# ------------------------------------------------------------------------------------------------- vt_fused_bias_act
MODES = ((1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2))


def fba_reference(x, b, r, step_b, act, grad, alpha, scale):
    """fused_bias_act_kernel.cu:40-61 in its order (add, select-multiply, multiply), in fp32 (double for fp64 tensors),
    rounded once to the tensor's dtype."""
    ct = F64 if x.dtype == F64 else F32
    v = x.to(ct)
    if b is not None:
        v = v + b.to(ct)[(torch.arange(x.numel()) // step_b) % b.numel()]
    a = torch.tensor(np.float32(alpha).item(), dtype=ct)
    mode = act * 10 + grad
    if mode in (12, 32):
        y = torch.zeros_like(v)
    elif mode == 30:
        y = torch.where(v > 0, v, v * a)
    elif mode == 31:
        y = torch.where((r.to(ct) if r is not None else torch.zeros_like(v)) > 0, v, v * a)
    else:
        y = v
    return (y * torch.tensor(np.float32(scale).item(), dtype=ct)).to(x.dtype)


def _fba_data(g, numel, step_b, size_b, dtype):
    x = rnd(g, (numel,), F32).to(dtype)
    b = rnd(g, (size_b,), F32).to(dtype)
    r = rnd(g, (numel,), F32).to(dtype)
    x[0], x[1 % numel] = -0.0, 0.0
    for i in range(2, min(numel, 12), 3):                 # x + b exactly 0
        x[i] = -b[(i // step_b) % size_b]
    r[3 % numel], r[4 % numel], r[(numel - 1)] = 0.0, -0.0, 0.0
    return x, b, r


def _fba_run(dev, x, b, r, step_b, act, grad, alpha, scale, offset=0):
    """Launch on views `offset` elements into their buffers; the output buffer is NaN around the view."""
    numel, dtype = x.numel(), x.dtype

    def place(t, fill):
        if t is None:
            return None
        buf = torch.full((t.numel() + offset + 8,), fill, dtype=dtype, device=dev)
        buf[offset:offset + t.numel()] = t.to(dev)
        return buf[offset:offset + t.numel()]
    obuf = torch.full((numel + offset + SLACK,), float("nan"), dtype=dtype, device=dev)
    out = obuf[offset:offset + numel]
    xd, bd, rd = place(x, 9.0), (None if b is None else b.to(dev)), place(r, 9.0)
    assert xd.data_ptr() % 16 == (offset * x.element_size()) % 16
    call("vt_fused_bias_act", out, xd, bd, rd, numel, step_b, 1 if b is None else b.numel(), act, grad, alpha, scale,
         DT[dtype], K._stream(obuf))
    sync(dev)
    assert_all_nan(obuf[:offset], "before the view")
    assert_all_nan(obuf[offset + numel:], "slack")
    return out


def _bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _assert_same_bits(got, want, what):
    if got.dtype == F64:
        bad = _bits64(got) != _bits64(want)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} fp64 elements differ"
    else:
        assert_bitwise(got, want, what)


@pytest.mark.parametrize("dtype", DTYPES + [F64])
def test_fused_bias_act_modes_and_forms(dev, dtype):
    """All six (act, grad) modes x bias x refer, bit-exact, in the three launch forms at their boundaries."""
    g = np.random.default_rng(108)
    vec = {F32: 4, BF16: 8, F16: 8, F64: 2}[dtype]
    big = 256 * vec * 4
    forms = [(1, 0, 0), (63, 0, 0), (64, 0, 0), (65, 0, 0), (67, 0, 0), (big, 0, 0), (big + vec, 0, 0),
             (64, 1, 0), (64 + vec, 3, 0), (64, 0, 5)]          # step_b, element offset of the views, numel % step_b
    if dtype == F64:
        forms = [(1, 0, 0), (64, 0, 0), (65, 1, 0), (64, 0, 5)]
    size_b = 3
    for step_b, offset, extra in forms:
        numel = 2 * size_b * step_b + extra
        x, b, r = _fba_data(g, numel, step_b, size_b, dtype)
        for act, grad in MODES:
            for use_b in (False, True):
                for use_r in (False, True):
                    alpha, scale = (0.2, 2 ** 0.5) if (act + grad + use_b) % 2 else (0.3, 0.7)
                    bb, rr = (b if use_b else None), (r if use_r else None)
                    got = _fba_run(dev, x, bb, rr, step_b, act, grad, alpha, scale, offset)
                    want = fba_reference(x, bb, rr, step_b, act, grad, alpha, scale)
                    _assert_same_bits(got, want, f"{dtype} step_b {step_b} offset {offset} numel {numel} mode {act}{grad} "
                                                 f"bias={use_b} refer={use_r}")


def _lrelu64(x, b, slope, scale):
    shape = [1, -1] + [1] * (x.ndim - 2)
    return F.leaky_relu(x + b.view(shape), slope) * scale


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_leaky_relu_gradients(dev, dtype):
    """op.fused_leaky_relu: first- and second-order gradients for x and bias per element against float64 autograd."""
    g = np.random.default_rng(109)
    for shape, slope, scale in (((3, 5, 8, 8), 0.2, 2 ** 0.5), ((2, 3, 5, 13), 0.1, 0.75), ((4, 6), 0.3, 1.25)):
        x = rnd(g, shape, F32).to(dtype)
        b = rnd(g, (shape[1],), F32).to(dtype)
        go, w1 = rnd(g, shape, F32).to(dtype), rnd(g, shape, F32).to(dtype)
        w2 = rnd(g, (shape[1],), F32).to(dtype)
        xd, bd, god = (t.to(dev).requires_grad_(True) for t in (x, b, go))
        out = op.fused_leaky_relu(xd, bd, slope, scale)
        gx, gb = torch.autograd.grad(out, (xd, bd), god, create_graph=True)
        (gg,) = torch.autograd.grad((gx * w1.to(dev)).sum() + (gb * w2.to(dev)).sum(), god)
        sync(dev)
        x6, b6, go6 = (t.double().requires_grad_(True) for t in (x, b, go))
        rx, rb = torch.autograd.grad(_lrelu64(x6, b6, slope, scale), (x6, b6), go6, create_graph=True)
        (rg,) = torch.autograd.grad((rx * w1.double()).sum() + (rb * w2.double()).sum(), go6)
        rx, rb = rx.detach(), rb.detach()
        case = f"{dtype} {shape} slope {slope} scale {scale}"
        tol_x = out_tol(rx, dtype, 2 * EPS * rx.abs())
        assert_close(gx, rx, tol_x, case + " grad x")
        dims = [0] + list(range(2, len(shape)))
        count = x.numel() // shape[1]
        tol_b = tol_x.sum(dims) + count * U * rx.abs().sum(dims)
        assert_close(gb, rb, out_tol(rb, dtype, tol_b), case + " grad bias")
        shape_b = [1, -1] + [1] * (len(shape) - 2)
        slack = 3 * EPS * (w1.double().abs() + w2.double().abs().view(shape_b)) * scale
        assert_close(gg, rg, out_tol(rg, dtype, slack), case + " second order")


# ------------------------------------------------------------------------------------------------ upfirdn2d gradients
def upfirdn_reference(x, k, up, down, pad):
    """Zero-insert, pad / crop, conv2d with the flipped kernel, decimate (op/upfirdn2d.py:168-199), differentiable."""
    n, c, h, w = x.shape
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    z = x.new_zeros((n, c, h, uy, w, ux))
    z[:, :, :, 0, :, 0] = x
    z = z.reshape(n, c, h * uy, w * ux)
    z = F.pad(z, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    z = z[:, :, max(-py0, 0):z.shape[2] - max(-py1, 0), max(-px0, 0):z.shape[3] - max(-px1, 0)]
    o = F.conv2d(z.reshape(n * c, 1, z.shape[2], z.shape[3]), torch.flip(k, [0, 1])[None, None])[:, :, ::dy, ::dx]
    return o.reshape(n, c, o.shape[2], o.shape[3])


FIR_32 = torch.tensor([[1.0, -2.0], [0.5, 3.0], [-0.25, 1.5]])          # 3 x 2, asymmetric, dyadic
FIR_14 = torch.tensor([[0.5, 1.0, -3.0, 0.25]])                         # 1 x 4
UPDOWN = ((1, 1), (2, 2), (1, 2), (2, 1))                               # (x, y)
PADS = ((2, 1, 0, 3), (-1, 2, 1, -1), (0, 3, 2, 0), (1, -2, -1, 2))


def _upfirdn_grad_case(dev, dtype, x, k, up, down, pad, exact, g):
    ref_out = upfirdn_reference(x.double(), k.double(), up, down, pad)
    go = torch.from_numpy(g.integers(-4, 5, tuple(ref_out.shape)).astype(np.float64)) if exact else \
        torch.from_numpy(g.standard_normal(tuple(ref_out.shape)))
    w = torch.from_numpy(g.integers(-3, 4, tuple(x.shape)).astype(np.float64)) if exact else \
        torch.from_numpy(g.standard_normal(tuple(x.shape)))
    xd, god = x.to(dev).requires_grad_(True), go.to(dtype).to(dev).requires_grad_(True)
    out = op.upfirdn2d(xd, k.to(dev), up, down, pad)
    (gx,) = torch.autograd.grad(out, xd, god, create_graph=True)
    (gg,) = torch.autograd.grad((gx * w.to(dtype).to(dev)).sum(), god)
    sync(dev)
    x6, go6 = x.double().requires_grad_(True), go.to(dtype).double().requires_grad_(True)
    r_out = upfirdn_reference(x6, k.double(), up, down, pad)
    (rx,) = torch.autograd.grad(r_out, x6, go6, create_graph=True)
    (rg,) = torch.autograd.grad((rx * w.to(dtype).double()).sum(), go6)
    case = f"{dtype} {tuple(x.shape)} fir {tuple(k.shape)} up {up} down {down} pad {pad}"
    assert tuple(out.shape) == tuple(r_out.shape), case
    if exact:
        _assert_same_bits(out.detach(), r_out.detach().to(dtype), case + " forward")
        _assert_same_bits(gx.detach(), rx.detach().to(dtype), case + " gradient")
        _assert_same_bits(gg, rg.to(dtype), case + " second order")
    else:       # VT_F64 on random data: 4 ulps of the absolute-value sum
        ka = k.double().abs()
        b_x = torch.autograd.grad(upfirdn_reference(x6, ka, up, down, pad), x6, go6.abs())[0]
        b_g = upfirdn_reference(w.double().abs(), ka, up, down, pad)
        assert_close(gx.detach(), rx.detach(), 4 * 2.0 ** -52 * b_x + 1e-300, case + " gradient")
        assert_close(gg, rg, 4 * 2.0 ** -52 * b_g + 1e-300, case + " second order")


@pytest.mark.parametrize("dtype", DTYPES + [F64])
def test_upfirdn2d_gradients(dev, dtype):
    """Gradient and second-order gradient per element: every up / down pairing, asymmetric FIRs, four-element pads with
    negative entries, sizes where the decimation leaves a remainder.  Integer data, dyadic taps: bit-exact."""
    g = np.random.default_rng(110)
    ran = ragged = 0
    for iu, up in enumerate(UPDOWN):
        for idn, down in enumerate(UPDOWN):
            for ik, k in enumerate((FIR_32, FIR_14)):
                for ip in range(2):
                    pad = PADS[(iu + idn + ik + 2 * ip) % 4]
                    h, w = (7, 9) if (iu + ip) % 2 == 0 else (6, 8)
                    x = torch.from_numpy(g.integers(-8, 9, (2, 2, h, w)).astype(np.float32)).to(dtype)
                    nh = h * up[1] + pad[2] + pad[3] - k.shape[0]
                    nw = w * up[0] + pad[0] + pad[1] - k.shape[1]
                    if nh < 0 or nw < 0:
                        continue
                    ragged += int(nh % down[1] != 0 or nw % down[0] != 0)
                    _upfirdn_grad_case(dev, dtype, x, k, up, down, pad, True, g)
                    ran += 1
    assert ran >= 56 and ragged >= 8, (ran, ragged)
    # a plane whose gradient (up = down = 1, 200 output columns) takes the wide-tile kernel
    x = torch.from_numpy(g.integers(-8, 9, (1, 2, 20, 200)).astype(np.float32)).to(dtype)
    _upfirdn_grad_case(dev, dtype, x, FIR_32, (1, 1), (1, 1), (2, 1, 0, 3), True, g)
    if dtype == F64:
        x = torch.from_numpy(g.standard_normal((2, 2, 7, 9)))
        k = torch.from_numpy(g.standard_normal((3, 2)))
        for up, down, pad in (((2, 1), (1, 2), PADS[0]), ((1, 2), (2, 1), PADS[1]), ((2, 2), (1, 1), PADS[2])):
            _upfirdn_grad_case(dev, dtype, x, k, up, down, pad, False, g)


# ---------------------------------------------------------------------------------------------------------- frame I/O
def pack_reference(frames, parsing, pscale, swap_rb):
    """oracle/frames_oracle.py pack_inputs with the swap optional and the parsing map multiplied by `pscale`."""
    f = frames[..., ::-1] if swap_rb else frames
    t = f.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)
    x = (t - np.float32(0.5)) / np.float32(0.5)
    if parsing is None:
        return x
    return np.concatenate([x, parsing.astype(np.float32) * np.float32(pscale)], 1)


def unpack_reference(img, swap_rb):
    """oracle/frames_oracle.py tensor2cv2: clip, (y + 1) * 127.5, truncate."""
    y = np.clip(img.astype(np.float32), np.float32(-1.0), np.float32(1.0))
    tmp = ((y.transpose(0, 2, 3, 1) + np.float32(1.0)) * np.float32(127.5)).astype(np.uint8)
    return tmp[..., ::-1] if swap_rb else tmp


FRAME_SHAPES = ((16, 17), (9, 29), (2, 7), (3, 5), (1, 1))          # h * w % 4 = 0, 1, 2, 3, 1


def _byte_view(t, offset, nbytes):
    return t[offset:offset + nbytes]


def test_frame_pack(dev):
    g = np.random.default_rng(111)
    n = 3
    for h, w in FRAME_SHAPES:
        hw = h * w
        frames = ((np.arange(n * hw * 3) * 37 + 11) % 256).astype(np.uint8)
        g.shuffle(frames)
        frames = frames.reshape(n, h, w, 3)
        for pc, pscale in ((0, 1.0), (1, 1 / 16), (4, 0.3), (19, 1 / 16)):
            parsing = g.standard_normal((n, pc, h, w)).astype(np.float32) * 5 if pc else None
            for swap in (0, 1):
                for off in ((0, 1) if hw % 4 == 0 else (0,)):      # a 1-byte offset forces the one-pixel form
                    fbuf = torch.zeros(n * hw * 3 + 8, dtype=torch.uint8)
                    fbuf[off:off + n * hw * 3] = torch.from_numpy(frames.reshape(-1))
                    fd = fbuf.to(dev)
                    ct = 3 + pc
                    x = nan_buf(n * ct * hw, F32, dev)
                    call("vt_frame_pack", x, fd[off:], swap, None if pc == 0 else torch.from_numpy(parsing).to(dev), pc,
                         pscale, n, h, w, K._stream(x))
                    sync(dev)
                    case = f"{h}x{w} pc{pc} swap{swap} offset{off}"
                    want = torch.from_numpy(np.ascontiguousarray(pack_reference(frames, parsing, pscale, swap)))
                    assert_bitwise(x[:n * ct * hw].view(n, ct, h, w), want, case)
                    assert_all_nan(x[n * ct * hw:], case)


def unpack_inputs():
    """For every u the fp32 boundary nearest u / 127.5 - 1 and its two neighbours, the clamp ends and beyond, zeros, infs."""
    b = (np.arange(256, dtype=np.float64) / 127.5 - 1.0).astype(np.float32)
    vals = np.concatenate([np.nextafter(b, np.float32(-np.inf)), b, np.nextafter(b, np.float32(np.inf)),
                           np.array([-1.0, 1.0, -1.5, 1.5, -100.0, 3e38, -3e38, 0.0, -0.0, np.inf, -np.inf], np.float32)])
    return vals.astype(np.float32)


def test_frame_unpack(dev):
    g = np.random.default_rng(112)
    n = 3
    vals = unpack_inputs()
    for h, w in ((16, 17), (9, 29), (2, 7), (3, 5), (1, 1), (20, 20)):
        hw = h * w
        img = vals[(np.arange(n * 3 * hw) * 7 + 3) % vals.size] if n * 3 * hw < vals.size else \
            np.concatenate([vals, g.uniform(-1.2, 1.2, n * 3 * hw - vals.size).astype(np.float32)])
        img = img.reshape(n, 3, h, w)
        for swap in (0, 1):
            for off in ((0, 1) if hw % 4 == 0 else (0,)):
                buf = torch.full((n * hw * 3 + off + SLACK,), 0xA5, dtype=torch.uint8, device=dev)
                call("vt_frame_unpack", buf[off:], torch.from_numpy(img).to(dev), swap, n, h, w, K._stream(buf))
                sync(dev)
                case = f"{h}x{w} swap{swap} offset{off}"
                want = torch.from_numpy(np.ascontiguousarray(unpack_reference(img, swap)))
                got = buf[off:off + n * hw * 3].cpu().view(n, h, w, 3)
                bad = got != want
                assert not bad.any(), f"{case}: {int(bad.sum())} bytes differ, first at {bad.nonzero()[0].tolist()}"
                assert bool((buf[:off].cpu() == 0xA5).all()) and bool((buf[off + n * hw * 3:].cpu() == 0xA5).all()), case
    assert set(unpack_reference(vals.reshape(1, 1, 1, -1).repeat(3, 1), 0).reshape(-1).tolist()) == set(range(256))


# --------------------------------------------------------------------------- vt_coords_from_flow, vt_convex_upsample
def convex_reference(flow, mask):
    """RAFT.upsample_flow (raft.py:72-84) in float64 -> (up, bar of the module docstring)."""
    n, _, h, w = flow.shape
    lg = mask.double().view(n, 1, 9, 8, 8, h, w)
    a = (lg - lg.amax(2, keepdim=True)).abs()
    wk = torch.softmax(lg, dim=2)
    uf = F.unfold(8 * flow.double(), [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    up = (wk * uf).sum(2)
    tol = ((16 + a) * EPS * (wk * uf).abs()).sum(2) + 1e-30
    shuffle = lambda t: t.permute(0, 1, 4, 2, 5, 3).reshape(n, 2, 8 * h, 8 * w)
    return shuffle(up), shuffle(tol)


def _coords_check(dev, flow):
    n, _, h, w = flow.shape
    coords = nan_buf(n * h * w * 2, F32, dev)
    call("vt_coords_from_flow", coords, flow, n, h, w, K._stream(coords))
    sync(dev)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=F64, device=flow.device), torch.arange(w, dtype=F64, device=flow.device),
                            indexing="ij")
    want = torch.stack([xs, ys], -1)[None] + flow.double().permute(0, 2, 3, 1)
    got = coords[:n * h * w * 2].view(n, h, w, 2).double()
    assert bool(((got - want).abs() <= U * want.abs()).all()), f"coords {n}x{h}x{w}"
    assert bool(torch.isnan(coords[n * h * w * 2:]).all())


def _convex_check(dev, flow, mask):
    n, _, h, w = flow.shape
    size = n * 2 * 64 * h * w
    up = nan_buf(size, F32, dev)
    call("vt_convex_upsample", up, flow, mask, n, h, w, K._stream(up))
    sync(dev)
    want, tol = convex_reference(flow, mask)
    got = up[:size].view(n, 2, 8 * h, 8 * w).double()
    bad = ~((got - want).abs() <= tol)
    assert not bool(bad.any()), f"convex {n}x{h}x{w}: {int(bad.sum())} of {bad.numel()} elements off"
    assert bool(torch.isnan(up[size:]).all())


def test_raft_glue_kernels(dev):
    g = np.random.default_rng(113)
    n = 3
    for h, w in ((1, 1), (1, 9), (8, 1), (5, 7), (46, 62)):
        flow = rnd(g, (n, 2, h, w), F32, 3.0).to(dev)
        _coords_check(dev, flow)
        mask = (rnd(g, (n, 576, h, w), F32, 30.0, 100.0)).to(dev)
        _convex_check(dev, flow, mask)
        _convex_check(dev, flow, rnd(g, (n, 576, h, w)).to(dev))          # unsaturated weights


# ------------------------------------------------------------------------------------- grid-stride passes (GPU only)
@pytest.mark.gpu
def test_grid_stride_affine_apply_fusion_pack(dev):
    """2 x 256^2 x 256 bf16: 4.2 M vectors (8.4 M with `other`), more than grid_for's 8192 x 256; bit-exact against the
    same fp32 element-wise operations done by torch on the device (one correctly rounded kernel each)."""
    if dev.type != "cuda":
        pytest.skip("GPU-only shape")
    n, hw, c = 2, 256 * 256, 256
    gen = torch.Generator(device=dev).manual_seed(30)
    x = torch.randn((n, hw, c), device=dev, generator=gen).to(BF16)
    o = torch.randn((n, hw, c), device=dev, generator=gen).to(BF16)
    scale = torch.randn((n, 2 * c), device=dev, generator=gen)
    shift = torch.randn((n, 2 * c), device=dev, generator=gen)
    out = nan_buf(n * hw * 2 * c, BF16, dev)
    call("vt_affine_apply", out, 2 * c, x, c, o, c, scale, shift, n, hw, c, DT[BF16], K._stream(out))
    sync(dev)
    v = torch.cat([x.float(), (x.float() - o.float()).abs()], -1)
    want = ((v * scale[:, None]) + shift[:, None]).to(BF16)
    assert torch.equal(out[:n * hw * 2 * c].view(n, hw, 2 * c).view(torch.int16), want.view(torch.int16))
    assert bool(torch.isnan(out[n * hw * 2 * c:]).all())
    del v, want, out
    skip = torch.randn((n, 3, hw), device=dev, generator=gen)
    mask = torch.rand((n, hw), device=dev, generator=gen)
    ld_out = 64 + c
    out = nan_buf(n * hw * ld_out, BF16, dev)
    call("vt_fusion_pack", out, ld_out, x, c, mask, skip, n, hw, c, DT[BF16], K._stream(out))
    sync(dev)
    want = torch.zeros((n, hw, ld_out), device=dev)
    want[..., :3] = skip.permute(0, 2, 1)
    want[..., 64:] = x.float() * mask[..., None]
    assert torch.equal(out[:n * hw * ld_out].view(n, hw, ld_out).view(torch.int16), want.to(BF16).view(torch.int16))
    assert bool(torch.isnan(out[n * hw * ld_out:]).all())


@pytest.mark.gpu
def test_grid_stride_fused_bias_act_flat(dev):
    """step_b = 63 keeps the flat form: 2.2 M + 5 elements, more than its 8192 x 256 cap."""
    if dev.type != "cuda":
        pytest.skip("GPU-only shape")
    g = np.random.default_rng(31)
    step_b, size_b = 63, 5
    numel = step_b * size_b * 7000 + 5
    x, b, r = _fba_data(g, numel, step_b, size_b, F32)
    for act, grad, use_r in ((3, 0, False), (3, 1, True)):
        got = _fba_run(dev, x, b, r if use_r else None, step_b, act, grad, 0.2, 2 ** 0.5)
        assert_bitwise(got, fba_reference(x, b, r if use_r else None, step_b, act, grad, 0.2, 2 ** 0.5), f"mode {act}{grad}")


@pytest.mark.gpu
def test_grid_stride_frame_io(dev):
    """4099 x 4099 (odd h * w: the one-pixel form): 16.8 M pixels, more than the 65536 x 256 cap of frame_io.hip."""
    if dev.type != "cuda":
        pytest.skip("GPU-only shape")
    g = np.random.default_rng(32)
    h = w = 4099
    hw = h * w
    frames = g.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    x = nan_buf(3 * hw, F32, dev)
    call("vt_frame_pack", x, torch.from_numpy(frames).to(dev), 1, None, 0, 1.0, 1, h, w, K._stream(x))
    sync(dev)
    want = torch.from_numpy(np.ascontiguousarray(pack_reference(frames, None, 1.0, 1)))
    assert torch.equal(x[:3 * hw].cpu().view(1, 3, h, w).view(torch.int32), want.view(torch.int32))
    assert bool(torch.isnan(x[3 * hw:]).all())
    img = g.uniform(-1.2, 1.2, (1, 3, h, w)).astype(np.float32)
    buf = torch.full((hw * 3 + SLACK,), 0xA5, dtype=torch.uint8, device=dev)
    call("vt_frame_unpack", buf, torch.from_numpy(img).to(dev), 1, 1, h, w, K._stream(buf))
    sync(dev)
    assert torch.equal(buf[:hw * 3].cpu().view(1, h, w, 3), torch.from_numpy(np.ascontiguousarray(unpack_reference(img, 1))))
    assert bool((buf[hw * 3:].cpu() == 0xA5).all())


@pytest.mark.gpu
def test_grid_stride_raft_glue(dev):
    """vt_coords_from_flow on 4099 x 4099 (16.8 M pixels) and vt_convex_upsample on 513 x 513 (16.84 M fine pixels, a 606 MB
    mask): both beyond the 65536 x 256 cap of flow_ops.hip; float64 references computed on the device."""
    if dev.type != "cuda":
        pytest.skip("GPU-only shape")
    gen = torch.Generator(device=dev).manual_seed(33)
    _coords_check(dev, torch.randn((1, 2, 4099, 4099), device=dev, generator=gen) * 3)
    flow = torch.randn((1, 2, 513, 513), device=dev, generator=gen) * 3
    mask = torch.randn((1, 576, 513, 513), device=dev, generator=gen) * 30 + 100
    _convex_check(dev, flow, mask)
