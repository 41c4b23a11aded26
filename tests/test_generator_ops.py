"""The kernels of include/vtoonify_amd_generator.h (csrc/generator_ops.hip, vtoonify_amd/generator.py), one by one against
restatements written out here in numpy / float64 from the header's text, in host emulation (CPU suite) and on the MI355X
(-m gpu).

Bounds.
  vt_philox_u32      integer arithmetic: equal words.  The three vectors are the known-answer tests that Random123 ships for
                     philox4x32-10 (kat_vectors); the numpy restatement below reproduces them too.
  vt_randn           1e-5 absolute against float64: |z| <= sqrt(48 ln 2) = 5.77, logf / sqrtf / sincosf are good to a few
                     float32 ulps (6e-8 relative each), the angle 6.2831855f v carries one more rounding of a value < 6.3
                     (4e-7 absolute, times r <= 5.77: 2.2e-6 at the very tail).
  vt_noise_bias_act  float32: four roundings (w n, + x, + bias, scale) of values no larger than m = |x| + |w n| + |bias|, each
                     2^-24 relative: |d| <= 1e-6 sqrt(2) m.  Relative to the RESULT no float32 evaluation can be bounded where
                     the three terms cancel; where they do not (|result| >= m / 2: five roundings of at most 2^-24 m each,
                     6e-7 of the result) the test also asserts |d| <= 1e-6 |result|.  bf16 / fp16 add one rounding of the result to the tensor's type: 2^-8 / 2^-11 of
                     |result| (the spacing of the format; half of it is the rounding itself), for fp16 at least the subnormal
                     spacing 2^-24.
  vt_lerp_rows       float32, (1 - f), two products, one sum: |d| <= 5e-7 (|a| + |b|) for 0 <= f <= 1; f = 0 and f = 1 exact.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from vtoonify_amd import _lib, generator as G

KEY = 0x0123456789ABCDEF
M32 = np.uint64(0xFFFFFFFF)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _err():
    return _lib.lib().vt_last_error().decode()


# ------------------------------------------------------------------------------------------------ restatements (numpy)
def philox_np(ctr_lo, ctr_hi, key):
    """Philox4x32-10 of the header: arrays of uint64 counters -> (n,4) uint32."""
    ctr_lo = np.atleast_1d(np.asarray(ctr_lo, dtype=np.uint64))
    ctr_hi = np.broadcast_to(np.asarray(ctr_hi, dtype=np.uint64), ctr_lo.shape)
    c0, c1 = ctr_lo & M32, ctr_lo >> np.uint64(32)
    c2, c3 = ctr_hi & M32, ctr_hi >> np.uint64(32)
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def randn_np(n, offset, key, stream_id):
    """Elements [offset, offset + n) of the header's normal sequence, in float64."""
    j0, j1 = offset // 4, (offset + n - 1) // 4
    w = philox_np(np.arange(j0, j1 + 1, dtype=np.uint64), np.uint64(stream_id), key).astype(np.float64)
    two_pi = np.float64(np.float32(2.0 * np.pi))          # the header's float32 constant, 6.2831855f
    z = np.empty((w.shape[0], 4))
    for p in (0, 1):
        u = (np.floor(w[:, 2 * p] / 256.0) + 1.0) * 2.0 ** -24
        v = np.floor(w[:, 2 * p + 1] / 256.0) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u))
        z[:, 2 * p] = r * np.cos(two_pi * v)
        z[:, 2 * p + 1] = r * np.sin(two_pi * v)
    return z.reshape(-1)[offset - 4 * j0: offset - 4 * j0 + n]


# --------------------------------------------------------------------------------------------------------- 1. Philox
KAT = [
    (0, 0, 0, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    # counter 243f6a88 85a308d3 13198a2e 03707344, key a4093822 299f31d0
    (0x85A308D3243F6A88, 0x0370734413198A2E, 0x299F31D0A4093822, "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def test_philox_known_answers(dev):
    for lo, hi, key, want in KAT:
        want = np.array([int(x, 16) for x in want.split()], dtype=np.uint32)
        assert (philox_np(lo, hi, key)[0] == want).all(), "the numpy restatement"
        assert (_words(G.philox_u32(1, lo, hi, key, dev))[0] == want).all(), hex(key)


def test_philox_blocks_follow_the_counter(dev):
    """Block i is counter ctr_lo + i with the carry into the high word of ctr_lo and none into ctr_hi; more than one workgroup."""
    lo, hi = 0x00000001FFFFFFF0, 0x0000000500000007
    got = _words(G.philox_u32(700, lo, hi, KEY, dev))
    want = philox_np(np.uint64(lo) + np.arange(700, dtype=np.uint64), np.uint64(hi), KEY)
    assert (got == want).all()
    wrap = _words(G.philox_u32(3, 0xFFFFFFFFFFFFFFFE, hi, KEY, dev))
    assert (wrap == philox_np(np.array([0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFFF, 0], dtype=np.uint64), np.uint64(hi), KEY)).all()


# ---------------------------------------------------------------------------------------------------------- 2. randn
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_randn_equals_definition(dev, n):
    for offset, stream_id in ((0, 0), (0, 7), (4 * 1000, 7), (4 * (1 << 31) + 2, 1 << 40), (5, 0)):
        got = G.randn(n, KEY, stream_id, dev, offset=offset).cpu().numpy().astype(np.float64)
        d = np.abs(got - randn_np(n, offset, KEY, stream_id)).max()
        assert d <= 1e-5, (n, offset, stream_id, d)


def test_randn_leaves_its_surroundings_alone(dev):
    """Lengths and offsets that end inside a block, into a buffer that is not 16-byte aligned: the neighbours keep their NaN."""
    for n, offset, shift in ((5, 0, 0), (5, 3, 0), (9, 0, 1), (1023, 2, 3), (8, 4, 0)):
        buf = torch.full((n + 16,), float("nan"), dtype=torch.float32, device=dev)
        view = buf[4 + shift: 4 + shift + n]
        _lib.check(_lib.lib().vt_randn(_ptr(view), n, offset, KEY, 3, ctypes.c_void_p(0)), "vt_randn")
        if dev.type == "cuda":
            torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.isnan(host[:4 + shift]).all() and np.isnan(host[4 + shift + n:]).all(), (n, offset, shift)
        assert np.abs(host[4 + shift: 4 + shift + n] - randn_np(n, offset, KEY, 3)).max() <= 1e-5


def test_randn_pieces_equal_the_whole(dev):
    whole = G.randn(1000, KEY, 2, dev)
    parts = torch.cat([G.randn(333, KEY, 2, dev), G.randn(7, KEY, 2, dev, offset=333), G.randn(660, KEY, 2, dev, offset=340)])
    assert torch.equal(whole, parts)
    assert not torch.equal(whole, G.randn(1000, KEY, 3, dev)) and not torch.equal(whole, G.randn(1000, KEY + 1, 2, dev))


def test_randn_statistics(dev):
    """One fixed draw of 2^20: every figure is a deterministic function of (KEY, stream 0)."""
    n = 1 << 20
    z = G.randn(n, KEY, 0, dev).cpu().numpy().astype(np.float64)
    assert np.abs(z - randn_np(n, 0, KEY, 0)).max() <= 1e-5
    mean, var = z.mean(), z.var()
    tail = (np.abs(z) > 3.0).mean()
    lag1 = np.corrcoef(z[:-1], z[1:])[0, 1]
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} P(|z|>3) {tail:.5f} lag1 {lag1:.3e} max|z| {np.abs(z).max():.3f}")
    assert abs(mean) <= 5 / np.sqrt(n)
    assert abs(var - 1) <= 5 * np.sqrt(2 / n)
    assert abs(tail - 0.0027) <= 2.5e-4
    assert abs(lag1) <= 5 / np.sqrt(n)
    assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(48 * np.log(2)) + 1e-5


def test_draw_noise(dev):
    """The noise of a forward call: seeded by torch's CPU generator, one stream per layer, element index (sample, pixel)."""
    assert G.noise_sizes(64) == [(4, 4), (8, 8), (8, 8), (16, 16), (16, 16), (32, 32), (32, 32), (64, 64), (64, 64)]
    assert len(G.noise_sizes(1024)) == 17 and G.noise_sizes(1024)[-1] == (1024, 1024)
    torch.manual_seed(11)
    a = G.draw_noise(2, 64, dev)
    state = torch.get_rng_state()
    b = G.draw_noise(2, 64, dev)
    torch.manual_seed(11)
    key = G.draw_key()
    assert torch.equal(torch.get_rng_state(), state), "one call consumes exactly one key's worth of the generator"
    c = G.draw_noise(2, 64, dev, key=key)
    assert [t.shape for t in a] == [(2, 1, h, w) for h, w in G.noise_sizes(64)]
    assert all(torch.equal(x, y) for x, y in zip(a, c)), "the same seed gives the same maps"
    assert all(not torch.equal(x, y) for x, y in zip(a, b)), "the next call draws another key"
    for i, t in enumerate(a):   # layer i = stream i; sample s = elements [s HW, (s+1) HW)
        hw = t[0].numel()
        assert torch.equal(t[1].reshape(-1), G.randn(hw, key, i, dev, offset=hw))
    # two layers of one size, and the two samples of one layer, are uncorrelated (N = 4096 pixels)
    top, below = a[8].cpu().numpy().astype(np.float64).reshape(2, -1), a[7].cpu().numpy().astype(np.float64).reshape(2, -1)
    n = top.shape[1]
    assert abs(np.corrcoef(top[0], below[0])[0, 1]) <= 5 / np.sqrt(n)
    assert abs(np.corrcoef(top[0], top[1])[0, 1]) <= 5 / np.sqrt(n)


# ------------------------------------------------------------------------------------------------- 3. noise_bias_act
NBA_SHAPES = [(2, 16, 512), (1, 15, 32), (3, 64, 64), (1, 4096, 40)]
DTYPES = {"f32": (torch.float32, _lib.VT_F32, 0.0, 0.0), "bf16": (torch.bfloat16, _lib.VT_BF16, 2.0 ** -8, 0.0),
          "f16": (torch.float16, _lib.VT_F16, 2.0 ** -11, 2.0 ** -24)}


def _nba_case(dev, shape, dt, nb_is_b, ld_extra, in_place, with_bias=True):
    B, HW, C = shape
    tdt, code, rel_out, abs_out = DTYPES[dt]
    g = torch.Generator().manual_seed(B * 1000 + HW + C)
    ld = C + ld_extra
    nb = B if nb_is_b else 1
    x = torch.randn((B, HW, C), generator=g).to(tdt)
    noise = torch.randn((nb, HW), generator=g)
    bias = torch.randn((C,), generator=g) * 0.5 if with_bias else None
    w = torch.tensor([0.37], dtype=torch.float32)
    guard = 64
    nan = float("nan")
    xbuf = torch.full((guard + B * HW * ld + guard,), nan, dtype=tdt)
    xbuf[guard: guard + B * HW * ld].view(B * HW, ld)[:, :C] = x.view(B * HW, C)
    d_x = xbuf.to(dev)
    d_o = d_x if in_place else torch.full_like(d_x, nan)
    d_noise, d_w, d_bias = noise.to(dev), w.to(dev), bias.to(dev) if with_bias else None
    rc = _lib.lib().vt_noise_bias_act(_ptr(d_o[guard:]), ld, _ptr(d_x[guard:]), ld, _ptr(d_noise), nb, _ptr(d_w),
                                      _ptr(d_bias) if with_bias else None, B, HW, C, code, ctypes.c_void_p(0))
    assert rc == 0, _err()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    host = d_o.cpu().to(torch.float64).numpy()
    body = host[guard: guard + B * HW * ld].reshape(B, HW, ld)
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + B * HW * ld:]).all(), "wrote outside the tensor"
    assert np.isnan(body[:, :, C:]).all(), "wrote into the row padding"
    x64 = x.to(torch.float64).numpy()
    t = np.float64(w.numpy()[0]) * noise.to(torch.float64).numpy()
    t = np.broadcast_to(t[:, :, None], (nb, HW, 1))
    b64 = bias.to(torch.float64).numpy() if with_bias else np.zeros(C)
    s = x64 + t + b64
    ref = np.where(s < 0, 0.2 * s, s) * np.sqrt(2.0)
    mag = (np.abs(x64) + np.abs(t) + np.abs(b64)) * np.sqrt(2.0)
    bound = 1e-6 * mag + rel_out * np.abs(ref) + abs_out
    excess = (np.abs(body[:, :, :C] - ref) - bound).max()
    assert excess <= 0, (shape, dt, nb, ld, in_place, excess)
    if dt == "f32":     # ... and relative to the result itself wherever the terms do not cancel (|result| at least half of m)
        plain = np.abs(ref) >= 0.5 * mag
        assert plain.any() and (np.abs(body[:, :, :C] - ref)[plain] <= 1e-6 * np.abs(ref)[plain]).all(), (shape, nb, ld)
    if not in_place:
        assert torch.equal(d_x.cpu().view(torch.uint8), xbuf.view(torch.uint8)), "the input changed"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", NBA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise_bias_act(dev, shape, dt):
    for nb_is_b in (False, True):
        _nba_case(dev, shape, dt, nb_is_b, ld_extra=0, in_place=False)
        _nba_case(dev, shape, dt, nb_is_b, ld_extra=16, in_place=True)
    _nba_case(dev, shape, dt, True, ld_extra=8, in_place=False, with_bias=False)


def test_noise_bias_act_wide_rows(dev):
    """More 16-byte vectors in a row than a workgroup has lanes (fp32, C = 1032: 258 vectors): the channel loop's second trip."""
    _nba_case(dev, (2, 9, 1032), "f32", True, ld_extra=8, in_place=False)


def test_noise_bias_act_adapter(dev):
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 8, 8, 16), generator=g).to(dev)
    noise = torch.randn((2, 1, 8, 8), generator=g).to(dev)
    bias = torch.randn((16,), generator=g).to(dev)
    w = torch.tensor([-0.6]).to(dev)
    want = torch.nn.functional.leaky_relu(x + w * noise.permute(0, 2, 3, 1) + bias, 0.2) * 2 ** 0.5
    got = G.noise_bias_act(x, noise, w, bias)
    assert (got - want).abs().max().item() <= 1e-5
    y = x.clone()
    assert G.noise_bias_act(y, noise, w, bias, out=y) is y and torch.equal(y, got)
    with pytest.raises(_lib.VtError):
        G.noise_bias_act(x, noise[:, :, :4], w, bias)


def test_noise_bias_act_refusals_launch_nothing(dev):
    L = _lib.lib()
    nan = float("nan")
    noise = torch.zeros((2, 16), device=dev)
    w = torch.ones((1,), device=dev)
    bias = torch.zeros((64,), device=dev)

    def call(what, rc_want, C=32, ld=40, nb=2, B=2, HW=16, dtype=_lib.VT_F32, x_off=0, x_ok=True, w_ok=True):
        x = torch.full((2 * 16 * 40 + 8,), 1.0, device=dev)
        out = torch.full((2 * 16 * 40 + 8,), nan, device=dev)
        rc = L.vt_noise_bias_act(_ptr(out), ld, _ptr(x[x_off:]) if x_ok else None, ld, _ptr(noise), nb, _ptr(w) if w_ok else None,
                                 _ptr(bias), B, HW, C, dtype, ctypes.c_void_p(0))
        msg = _err()
        assert rc == rc_want and "vt_noise_bias_act" in msg, (what, rc, msg)
        assert torch.isnan(out.cpu()).all(), f"{what}: a kernel ran"
        return msg

    assert "multiple of 8" in call("C = 36", 2, C=36)
    assert "multiple of 8" in call("C = 4", 2, C=4)
    assert "dtype" in call("double", 2, dtype=_lib.VT_F64)
    assert "neither 1 nor B" in call("noise batch 3", 1, nb=3)
    assert "row stride" in call("ld below C", 1, C=32, ld=24)
    assert "aligned" in call("ld not a multiple of 16 bytes", 1, C=32, ld=34)
    assert "aligned" in call("pointer not 16-byte aligned", 1, x_off=1)
    call("null x", 1, x_ok=False)
    call("null weight", 1, w_ok=False)
    call("empty batch", 1, B=0, nb=0)
    call("empty plane", 1, HW=0)


# ---------------------------------------------------------------------------------------------------------- 4. lerp_rows
@pytest.mark.parametrize("rows", [1, 20])
def test_lerp_rows(dev, rows):
    g = torch.Generator().manual_seed(rows)
    a = torch.randn((rows, 512), generator=g)
    b = torch.randn((rows, 512), generator=g)
    a64, b64 = a.to(torch.float64).numpy(), b.to(torch.float64).numpy()
    tol = 5e-7 * (np.abs(a64) + np.abs(b64))
    for f in (torch.tensor([0.7]), torch.rand((rows,), generator=g)):
        got = G.lerp_rows(a.to(dev), b.to(dev), f.to(dev)).cpu().to(torch.float64).numpy()
        f64 = f.to(torch.float64).numpy().reshape(-1, 1)
        assert (np.abs(got - (f64 * b64 + (1 - f64) * a64)) <= tol).all()
    # the ends are exact, as one factor and among per-row factors
    assert torch.equal(G.lerp_rows(a.to(dev), b.to(dev), torch.zeros(1).to(dev)).cpu(), a)
    assert torch.equal(G.lerp_rows(a.to(dev), b.to(dev), torch.ones(1).to(dev)).cpu(), b)
    f = torch.tensor([0.0, 1.0] * rows)[:rows]
    got = G.lerp_rows(a.to(dev), b.to(dev), f.to(dev)).cpu()
    assert torch.equal(got[0::2], a[0::2]) and torch.equal(got[1::2], b[1::2])
    # truncation: one latent row against every style row, in place over the styles
    mean = torch.randn((1, 512), generator=g)
    styles = b.clone().to(dev)
    G.lerp_rows(mean.to(dev), styles, torch.tensor([0.5]).to(dev), out=styles)
    want = 0.5 * b64 + 0.5 * mean.to(torch.float64).numpy()
    assert np.abs(styles.cpu().to(torch.float64).numpy() - want).max() <= 1e-6
    # (B, n_latent, 512) latents with a per-row factor
    if rows == 20:
        got = G.lerp_rows(a.view(2, 10, 512).to(dev), b.view(2, 10, 512).to(dev), torch.rand((20,), generator=g).to(dev))
        assert got.shape == (2, 10, 512)


def test_lerp_rows_refusals_launch_nothing(dev):
    L = _lib.lib()
    a = torch.zeros((4, 16), device=dev)
    f = torch.zeros((4,), device=dev)

    def call(what, ld_out=16, ld_a=16, ld_b=16, f_stride=1, rows=4, dim=16, f_ok=True):
        out = torch.full((4, 16), float("nan"), device=dev)
        rc = L.vt_lerp_rows(_ptr(out), ld_out, _ptr(a), ld_a, _ptr(a), ld_b, _ptr(f) if f_ok else None, f_stride, rows, dim,
                            ctypes.c_void_p(0))
        msg = _err()
        assert rc == 1 and "vt_lerp_rows" in msg, (what, rc, msg)
        assert torch.isnan(out.cpu()).all(), f"{what}: a kernel ran"

    call("output stride below dim", ld_out=8)
    call("input stride between 0 and dim", ld_a=8)
    call("factor stride 2", f_stride=2)
    call("no rows", rows=0)
    call("no columns", dim=0)
    call("null factor", f_ok=False)
    with pytest.raises(_lib.VtError):
        G.lerp_rows(a, torch.zeros((3, 16), device=dev), f)


def test_randn_philox_refusals(dev):
    L = _lib.lib()
    out = torch.full((8,), float("nan"), device=dev)
    s = ctypes.c_void_p(0)
    assert L.vt_randn(_ptr(out), -1, 0, 1, 0, s) == 1 and "vt_randn" in _err()
    assert L.vt_randn(_ptr(out), 4, -4, 1, 0, s) == 1 and "vt_randn" in _err()
    assert L.vt_randn(None, 4, 0, 1, 0, s) == 1 and "vt_randn" in _err()
    assert L.vt_philox_u32(None, 1, 0, 0, 0, s) == 1 and "vt_philox_u32" in _err()
    assert L.vt_philox_u32(_ptr(out), -1, 0, 0, 0, s) == 1 and "vt_philox_u32" in _err()
    assert L.vt_randn(_ptr(out), 0, 0, 1, 0, s) == 0 and L.vt_philox_u32(_ptr(out), 0, 0, 0, 0, s) == 0
    assert torch.isnan(out.cpu()).all()


# ----------------------------------------------------------------------------------- 5. declaration, binding and export
def test_generator_header_binding_and_export():
    """include/vtoonify_amd_generator.h as tests/test_face_align.py treats its header: what it declares is what _lib binds (its
    own dict), the gfx950 library exports it, the main header includes it and declares none of it itself."""
    from vtoonify_amd import build
    src = open(os.path.join(REPO, "include", "vtoonify_amd_generator.h")).read()
    declared = sorted(set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.GENERATOR_SYMBOLS) == ["vt_lerp_rows", "vt_noise_bias_act", "vt_philox_u32", "vt_randn"]
    others = set(_lib.EXPORTED_SYMBOLS) | set(_lib.PREPASS_SYMBOLS) | set(_lib.FRAMES_SYMBOLS) | set(_lib.FUSION_SYMBOLS) | \
        set(_lib.RGBUP_SYMBOLS) | set(_lib.ALIGN_SYMBOLS)
    assert not set(declared) & others
    main = open(os.path.join(REPO, "include", "vtoonify_amd.h")).read()
    assert '#include "vtoonify_amd_generator.h"' in main
    assert not set(declared) & set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", main))
    assert "generator_ops.hip" in build.SOURCES and _lib.ABI_VERSION == 5
    lib = ctypes.CDLL(build.build(verbose=False))
    kind_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_int64: "q", ctypes.c_uint64: "Q"}
    for name in declared:
        assert hasattr(lib, name), name
        decl = re.search(r"^int %s\(([^)]*)\)" % name, src, re.M)
        res, args = _lib._GENERATOR_SIGS[name]
        assert res is ctypes.c_int
        kinds = []
        for arg in decl.group(1).split(","):
            if "*" in arg or "vt_stream" in arg:
                kinds.append("p")
            elif "uint64_t" in arg:
                kinds.append("Q")
            else:
                kinds.append("q" if "int64_t" in arg else "i")
        assert [kind_of[t] for t in args] == kinds, (name, kinds)
