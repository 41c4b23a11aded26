"""Face alignment for the style encoder from given landmarks: vtoonify_amd/align.py, csrc/face_align.hip and
include/vtoonify_amd_align.h, in host emulation (CPU suite) and on the MI355X (-m gpu).

References: tests/golden/align.npz holds what the reference's own align_face (Pillow, scipy) returns for the cases of
tests/align_cases.py (tests/golden/make_golden_align.py); the kernels are also held against restatements written out here in
plain numpy from the formulas of DESIGN.md 4.9, independent of vtoonify_amd/align.py.

Bounds.  Shrink and transform are integer / float64 arithmetic that Pillow fixes completely: 0 differing bytes.  The pad
branch is float32 with a float64-accumulated blur; a value that differs in its last float32 bit can flip one level at the
uint8 rounding, which stays <= 1 through the convex bilinear combination and the truncation of the transform: max |diff| <= 1
and at most 1e-3 of the values (float32 accumulation of the blur was seen at 2.4e-4; this implementation gives 0).
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import align_cases as AC
from conftest import REPO, load_golden
from vtoonify_amd import _lib, align as A

GOLD, META = load_golden("align.npz")
SENT = 0xAB


def _plan(name):
    return A.align_parameters(AC.lm_of(name), AC.CASES[name][:2])


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _err():
    return _lib.lib().vt_last_error().decode()


# --------------------------------------------------------------------------------------------------------------- 1. plan
def test_plan_equals_reference():
    AC.check_branches(A.align_parameters)
    for name in AC.CASES:
        img, lm = AC.case(name)
        assert [AC.crc(img), AC.crc(lm)] == GOLD[f"{name}__crc"].tolist(), f"{name}: the inputs are not the fixture's"
        p = _plan(name)
        g = GOLD[f"{name}__plan"].tolist()
        shrink, rsize, cropped, crop, padded, pad, size = g[0], tuple(g[1:3]), g[3], tuple(g[4:8]), g[8], tuple(g[9:13]), tuple(g[13:15])
        assert p.shrink == shrink and type(p.shrink) is int
        assert (p.rsize is not None) == (shrink > 1) and (p.rsize is None or p.rsize == rsize)
        assert (p.crop is not None) == bool(cropped) and (p.crop is None or p.crop == crop)
        assert (p.pad is not None) == bool(padded) and (p.pad is None or p.pad == pad)
        assert p.size == size
        q = GOLD[f"{name}__quad"]
        assert np.all(np.abs(p.quad - q) <= 1e-12 * np.maximum(np.abs(q), 1.0)), name
    H, W, centre, d, tilt = AC.TOO_LARGE
    with pytest.raises(ValueError, match="reaches the side"):
        A.align_parameters(AC.landmarks(centre, d, tilt), (H, W))
    with pytest.raises(ValueError, match=r"\(68,2\)"):
        A.align_parameters(np.zeros((5, 2)), (64, 64))
    # float landmarks (--landmarks) are taken as given
    assert A.align_parameters(AC.lm_of("inside").astype(np.float64), (360, 480)).crop == _plan("inside").crop


# ---------------------------------------------------------------------------------------------------------- 2. transform
def ref_quad(img, a, S):
    """Pillow's QUAD + BILINEAR, one pixel at a time, in Python floats (float64)."""
    h, w = img.shape[:2]
    out = np.zeros((S, S, 3), dtype=np.uint8)
    for y in range(S):
        for x in range(S):
            xo, yo = x + 0.5, y + 0.5
            xin = a[0] + a[1] * xo + a[2] * yo + a[3] * xo * yo
            yin = a[4] + a[5] * xo + a[6] * yo + a[7] * xo * yo
            if xin < 0.0 or xin >= w or yin < 0.0 or yin >= h:
                continue
            xin, yin = xin - 0.5, yin - 0.5
            ix, iy = math.floor(xin), math.floor(yin)
            dx, dy = xin - ix, yin - iy
            x0, x1 = min(max(ix, 0), w - 1), min(max(ix + 1, 0), w - 1)
            y0, y1 = min(max(iy, 0), h - 1), min(max(iy + 1, 0), h - 1)
            for c in range(3):
                p00, p01, p10, p11 = (float(img[y0, x0, c]), float(img[y0, x1, c]), float(img[y1, x0, c]), float(img[y1, x1, c]))
                v1 = p00 + (p01 - p00) * dx
                v2 = p10 + (p11 - p10) * dx
                out[y, x, c] = int(v1 + (v2 - v1) * dy)
    return out


def _normalised(u8):
    t = torch.from_numpy(u8).permute(2, 0, 1)[None].to(torch.float32)          # torch float32 on the host: a true division
    return ((t / 255.0) - 0.5) / 0.5


def test_quad_bit_exact(dev):
    for name in AC.NO_PAD:
        img, _ = AC.case(name)
        p = _plan(name)
        x0, y0, x1, y1 = p.crop
        rows = torch.from_numpy(img[y0:y1].copy()).to(dev)                   # the crop is a view: offset and pitch, no copy
        u8, x = A.quad_transform(rows, 3 * x0, y1 - y0, x1 - x0, 3 * img.shape[1], A.quad_coefficients(p.quad, 256))
        got = u8.cpu().numpy()
        assert int((got != GOLD[f"{name}__out"]).sum()) == 0, name
        assert torch.equal(x.cpu(), _normalised(got)), name
    # a small output whose quad lies partly outside a 5 x 7 image: zeros outside, the float64 formula inside
    g = np.random.default_rng(3)
    img = g.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    quad = np.array([[-2.3, -1.1], [-1.2, 5.4], [6.1, 6.3], [8.2, -0.4]])
    a = A.quad_coefficients(quad, 8)
    want = ref_quad(img, a, 8)
    outside = (want == 0).all(axis=2)
    assert 8 < outside.sum() < 56
    u8, x = A.quad_transform(torch.from_numpy(img).to(dev), 0, 5, 7, 21, a, size=8)
    assert np.array_equal(u8.cpu().numpy(), want) and np.array_equal(A.quad_host(img, a, 8), want)
    assert torch.equal(x.cpu(), _normalised(want)) and (x.cpu()[0, :, torch.from_numpy(outside)] == -1).all()
    u8b, none = A.quad_transform(torch.from_numpy(img).to(dev), 0, 5, 7, 21, a, size=8, normalised=False)
    assert none is None and torch.equal(u8b.cpu(), u8.cpu())


# ----------------------------------------------------------------------------------------------------------- 3. resample
def ref_lanczos(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for LANCZOS, one output index at a time."""
    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(v * math.pi) / (v * math.pi)

    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    tab = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        k = []
        for v in range(xmin, xmax):
            t = (v - center + 0.5) / fs
            k.append(sinc(t) * sinc(t / 3.0) if -3.0 <= t < 3.0 else 0.0)
        ww = 0.0
        for v in k:
            ww += v
        k = [v / ww for v in k]
        tab.append((xmin, [int(v * 2 ** 22 - 0.5) if v < 0 else int(v * 2 ** 22 + 0.5) for v in k]))
    return tab


def ref_resize(img, size):
    """Image.resize(size, LANCZOS) on 8-bit RGB from the integer formula: horizontal pass, uint8, vertical pass."""
    def one(P, tab):                          # along axis 1
        out = np.zeros((P.shape[0], len(tab), 3), dtype=np.uint8)
        for j, (first, k) in enumerate(tab):
            acc = (1 << 21) + (P[:, first:first + len(k)].astype(np.int64) * np.array(k, dtype=np.int64)[None, :, None]).sum(axis=1)
            out[:, j] = np.clip(acc >> 22, 0, 255)
        return out

    T = one(img, ref_lanczos(img.shape[1], size[0]))
    return one(T.transpose(1, 0, 2), ref_lanczos(img.shape[0], size[1])).transpose(1, 0, 2)


_RESIZED = {}


def _resized(name):
    if name not in _RESIZED:
        img, _ = AC.case(name)
        r = ref_resize(img, _plan(name).rsize)
        r.setflags(write=False)
        _RESIZED[name] = (img, r)
    return _RESIZED[name]


def _resample(dev, img, rsize, x0, y0, x1, y1):
    H, W = img.shape[:2]
    xb, xk = A.lanczos_tables(W, rsize[0], x0, x1)
    yb, yk = A.lanczos_tables(H, rsize[1], y0, y1)
    r0, r1 = int(yb[:, 0].min()), int((yb[:, 0] + yb[:, 1]).max())
    out = A.resample(torch.from_numpy(img[r0:r1].copy()).to(dev), r0, H, xb, xk, yb, yk).cpu().numpy()
    assert np.array_equal(A.resample_host(img, 0, xb, xk, yb, yk), out)
    return out, (r0, r1)


def test_resample_bit_exact(dev):
    for name in ("shrink2", "shrink3"):
        img, want = _resized(name)
        rs = _plan(name).rsize
        got, rows = _resample(dev, img, rs, 0, 0, rs[0], rs[1])
        assert got.shape == want.shape == (rs[1], rs[0], 3) and int((got != want).sum()) == 0, name
        assert rows == (0, img.shape[0])
    # a sub-rectangle equals the slice of the full result, and reads a slab of the source only
    img, want = _resized("shrink3")
    got, (r0, r1) = _resample(dev, img, (256, 213), 37, 50, 150, 121)
    assert np.array_equal(got, want[50:121, 37:150]) and r0 > 0 and r1 < img.shape[0]


def test_resample_equals_pillow(dev):
    Image = pytest.importorskip("PIL.Image", reason="Pillow not importable: the integer formula stays the only reference")
    for name in ("shrink2", "shrink3"):
        img, want = _resized(name)
        rs = _plan(name).rsize
        pil = np.asarray(Image.fromarray(img).resize(rs, Image.LANCZOS))
        assert int((pil != want).sum()) == 0, name
    img = AC.image(375, 500, 9)                               # 1500x1125 / 3, / 4.5: a non-integer factor on one axis
    for rs in ((250, 125), (111, 83)):
        got, _ = _resample(dev, img, rs, 0, 0, rs[0], rs[1])
        assert int((np.asarray(Image.fromarray(img).resize(rs, Image.LANCZOS)) != got).sum()) == 0, rs


# ---------------------------------------------------------------------------------------------------------- 4. pad blend
def ref_pad_blend(view, pad, r, taps):
    """align_all_parallel.py:133-141 in explicit float32 numpy; the blur sums a line in float64 (centre, then pairs from
    the outermost inwards) over a 'symmetric' extension, np.median is the exact median."""
    f32 = np.float32
    pl, pt, pr, pb = pad
    img = np.pad(view.astype(f32), ((pt, pb), (pl, pr), (0, 0)), "reflect")
    h, w, _ = img.shape
    mask = np.zeros((h, w, 1), dtype=f32)
    for y in range(h):
        for x in range(w):
            mx = min(f32(x) / f32(pl), f32(w - 1 - x) / f32(pr))
            my = min(f32(y) / f32(pt), f32(h - 1 - y) / f32(pb))
            mask[y, x, 0] = max(f32(1) - mx, f32(1) - my)
    blur = img
    for axis in (0, 1):
        ext = np.pad(blur.astype(np.float64), [(r, r) if a == axis else (0, 0) for a in range(3)], "symmetric")
        ext = np.moveaxis(ext, axis, 0)
        n = blur.shape[axis]
        acc = ext[r:r + n] * taps[0]
        for j in range(r, 0, -1):
            acc = acc + (ext[r - j:r - j + n] + ext[r + j:r + j + n]) * taps[j]
        blur = np.moveaxis(acc, 0, axis).astype(f32)
    img = img + (blur - img) * np.clip(mask * f32(3) + f32(1), f32(0), f32(1))
    med = np.median(img, axis=(0, 1))
    assert img.dtype == f32 and med.dtype == f32
    img = img + (med - img) * np.clip(mask, f32(0), f32(1))
    assert img.dtype == f32
    return np.uint8(np.clip(np.rint(img), 0, 255))


def test_pad_blend(dev):
    # the median and the blends on a small view cut out of a larger image: an even (12 x 18) and an odd (13 x 19) pixel count
    big = AC.image(20, 30, 11)
    taps = A.gaussian_taps(0.55)
    assert len(taps) == 3
    for (h0, w0) in ((9, 11), (10, 12)):
        view = big[4:4 + h0, 6:6 + w0]
        want = ref_pad_blend(view, (3, 2, 4, 1), 2, taps)
        assert (want.shape[0] * want.shape[1]) % 2 == (0 if (h0, w0) == (9, 11) else 1)
        got = A.pad_blend(torch.from_numpy(big).to(dev), (4 * 30 + 6) * 3, h0, w0, 90, (3, 2, 4, 1), taps).cpu().numpy()
        assert np.array_equal(got, want), (h0, w0, int((got != want).sum()))
        assert np.array_equal(A.pad_blend_host(view, (3, 2, 4, 1), taps), want)
    # end to end against the reference's crops
    fa = A.FaceAligner(dev)
    for name in AC.PADDED:
        img, lm = AC.case(name)
        u8, x = fa(img, lm)
        got = u8.cpu().numpy()
        d = np.abs(got.astype(np.int32) - GOLD[f"{name}__out"].astype(np.int32))
        print(f"[align] {name} on {dev}: max |diff| = {int(d.max())}, share of differing values = {float((d > 0).mean()):.3g}")
        assert int(d.max()) <= 1 and float((d > 0).mean()) <= 1e-3, name
        assert tuple(x.shape) == (1, 3, 256, 256) and torch.equal(x.cpu(), _normalised(got))
    # a frame that is already on the device gives the same crop
    img, lm = AC.case("corner")
    u8b, _ = fa(torch.from_numpy(img).to(dev), lm)
    assert torch.equal(u8b.cpu(), fa(img, lm)[0].cpu())


def test_host_form_equals_goldens():
    for name in AC.CASES:
        img, lm = AC.case(name)
        got = A.align_face_host(img, lm)
        d = np.abs(got.astype(np.int32) - GOLD[f"{name}__out"].astype(np.int32))
        if name in AC.NO_PAD:
            assert int((d > 0).sum()) == 0, name
        else:
            print(f"[align] {name} host form: max |diff| = {int(d.max())}, share = {float((d > 0).mean()):.3g}")
            assert int(d.max()) <= 1 and float((d > 0).mean()) <= 1e-3, name
    x = A.normalise_host(GOLD["tiny__out"])
    assert x.dtype == np.float32 and np.array_equal(x, _normalised(GOLD["tiny__out"]).numpy())
    with pytest.raises(ValueError):
        A.align_face_host(np.zeros((64, 64), dtype=np.uint8), AC.lm_of("tiny"))


# ------------------------------------------------------------------------------------------------- 5. errors, not faults
def test_inconsistent_arguments_are_errors_and_launch_nothing(dev):
    L = _lib.lib()
    stream = ctypes.c_void_p(0)
    img = AC.image(40, 52, 13)
    d_img = torch.from_numpy(img).to(dev)

    # ---- vt_align_resample_u8: 40x52 -> 20x26
    xb, xk = A.lanczos_tables(52, 26)
    yb, yk = A.lanczos_tables(40, 20)

    def resample(what, rc_want=1, rows=40, row0=0, xb=xb, xk=xk, yb=yb, yk=yk, kx=None, ky=None, src=d_img):
        out = torch.full((20, 26, 3), SENT, dtype=torch.uint8, device=dev)
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in (xb, xk, yb, yk)]
        rc = L.vt_align_resample_u8(_ptr(out), _ptr(src) if src is not None else None, rows, row0, 40, 52, _ptr(t[0]), _ptr(t[1]),
                                    xk.shape[1] if kx is None else kx, _ptr(t[2]), _ptr(t[3]), yk.shape[1] if ky is None else ky,
                                    20, 26, stream)
        msg = _err()
        assert rc == rc_want and "vt_align_resample_u8" in msg, (what, rc, msg)
        assert (out.cpu() == SENT).all(), f"{what}: a kernel ran"
        return msg

    bad = xb.copy()
    bad[7, 0] = 52 - bad[7, 1] + 1
    assert "xbound[7]" in resample("a column index leaves the image", xb=bad)
    bad = yb.copy()
    bad[3, 0] = -1
    assert "ybound[3]" in resample("a row index below 0", yb=bad)
    bad = xb.copy()
    bad[2, 1] = xk.shape[1] + 1
    assert "xbound[2]" in resample("a count beyond the table width", xb=bad)
    assert "ybound" in resample("a table narrower than its counts", ky=yk.shape[1] - 1)
    assert "slab" in resample("a row outside the slab", rows=39, row0=1, src=d_img[1:].contiguous())
    resample("slab past the image", rows=40, row0=1)
    resample("null source", src=None)
    # shrink factors whose footprint does not fit the smallest tile: unsupported, named
    big_xb, big_xk = np.array([[0, 4000]] * 26, dtype=np.int32), np.ones((26, 4000), dtype=np.int32)
    wide = torch.zeros((40, 4000, 3), dtype=torch.uint8, device=dev)
    out = torch.full((20, 26, 3), SENT, dtype=torch.uint8, device=dev)
    t = [torch.from_numpy(a).to(dev) for a in (big_xb, big_xk, yb, yk)]
    rc = L.vt_align_resample_u8(_ptr(out), _ptr(wide), 40, 0, 40, 4000, _ptr(t[0]), _ptr(t[1]), 4000, _ptr(t[2]), _ptr(t[3]),
                                yk.shape[1], 20, 26, stream)
    assert rc == 2 and "LDS" in _err() and (out.cpu() == SENT).all()

    # ---- vt_align_pad_blend: a 9x11 view of the image
    taps = torch.from_numpy(A.gaussian_taps(0.55)).to(dev)
    need = int(L.vt_align_pad_blend_workspace(12, 18, 2))
    assert need >= 2 * 12 * 18 * 3 * 4
    assert L.vt_align_pad_blend_workspace(0, 18, 2) == 0 and "vt_align_pad_blend_workspace" in _err()

    def blend(what, rc_want=1, pads=(3, 2, 4, 1), r=2, ws_bytes=None, ws_ok=True):
        out = torch.full((12, 18, 3), SENT, dtype=torch.uint8, device=dev)
        ws = torch.full((need,), SENT, dtype=torch.uint8, device=dev)
        rc = L.vt_align_pad_blend(_ptr(out), _ptr(d_img), 9, 11, 156, *pads, _ptr(taps), r, _ptr(ws) if ws_ok else None,
                                  need if ws_bytes is None else ws_bytes, stream)
        msg = _err()
        assert rc == rc_want and "vt_align_pad_blend" in msg, (what, rc, msg)
        assert (out.cpu() == SENT).all() and (ws.cpu() == SENT).all(), f"{what}: a kernel ran"
        return msg

    assert "divides" in blend("a pad of 0", pads=(3, 0, 4, 1))
    assert "reflect" in blend("a pad as wide as the view", pads=(11, 2, 4, 1))
    assert "reflect" in blend("a pad as high as the view", pads=(3, 2, 4, 9))
    assert "radius" in blend("a negative radius", r=-1)
    assert "radius" in blend("a radius that reaches the padded side", r=12)
    assert "workspace" in blend("a workspace one byte short", ws_bytes=need - 1)
    blend("no workspace", ws_ok=False)
    # a radius beyond the halo that the row blur holds in LDS: unsupported (180 x 180 padded, radius 129; nothing is read)
    src = torch.zeros((100, 100, 3), dtype=torch.uint8, device=dev)
    out = torch.full((180, 180, 3), SENT, dtype=torch.uint8, device=dev)
    ws = torch.full((1 << 20,), SENT, dtype=torch.uint8, device=dev)
    rc = L.vt_align_pad_blend(_ptr(out), _ptr(src), 100, 100, 300, 40, 40, 40, 40, _ptr(taps), 129, _ptr(ws), 1 << 20, stream)
    assert rc == 2 and "vt_align_pad_blend: radius 129" in _err() and (out.cpu() == SENT).all() and (ws.cpu() == SENT).all()
    assert L.vt_align_pad_blend_workspace(180, 180, 129) == 0

    # ---- vt_align_quad
    a = A.quad_coefficients(np.array([[1.0, 1.0], [1.0, 30.0], [40.0, 30.0], [40.0, 1.0]]), 8)

    def quad(what, h=40, w=52, pitch=156, S=8, a=a, src=d_img):
        u8 = torch.full((8, 8, 3), SENT, dtype=torch.uint8, device=dev)
        f = torch.full((3, 8, 8), float("nan"), dtype=torch.float32, device=dev)
        coef = (ctypes.c_double * 8)(*a)
        rc = L.vt_align_quad(_ptr(u8), _ptr(f), _ptr(src) if src is not None else None, h, w, pitch, coef, S, stream)
        msg = _err()
        assert rc == 1 and "vt_align_quad" in msg, (what, rc, msg)
        assert (u8.cpu() == SENT).all() and torch.isnan(f.cpu()).all(), f"{what}: a kernel ran"

    quad("pitch below a row", pitch=155)
    quad("empty output", S=0)
    quad("empty view", h=0)
    quad("null image", src=None)
    nan = a.copy()
    nan[5] = float("nan")
    quad("a coefficient that is not a number", a=nan)
    inf = a.copy()
    inf[0] = float("inf")
    quad("an infinite coefficient", a=inf)

    # the plan raises what the entry would refuse, and the adapter raises on a frame it cannot take
    with pytest.raises(ValueError):
        A.align_parameters(AC.landmarks(*AC.TOO_LARGE[2:]), AC.TOO_LARGE[:2])
    with pytest.raises(_lib.VtError):
        A.FaceAligner(dev)(np.zeros((64, 80, 3), dtype=np.float32), AC.lm_of("tiny"))


def test_align_header_binding_and_export():
    """include/vtoonify_amd_align.h as tests/test_frame_scale.py treats the frames header: what it declares is what _lib binds
    (its own dict), the gfx950 library exports it, the main header includes it."""
    from vtoonify_amd import build
    src = open(os.path.join(REPO, "include", "vtoonify_amd_align.h")).read()
    declared = sorted(set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.ALIGN_SYMBOLS) == ["vt_align_pad_blend", "vt_align_pad_blend_workspace", "vt_align_quad",
                                                      "vt_align_resample_u8"]
    others = set(_lib.EXPORTED_SYMBOLS) | set(_lib.PREPASS_SYMBOLS) | set(_lib.FRAMES_SYMBOLS) | set(_lib.FUSION_SYMBOLS) | \
        set(_lib.RGBUP_SYMBOLS)
    assert not set(declared) & others
    assert '#include "vtoonify_amd_align.h"' in open(os.path.join(REPO, "include", "vtoonify_amd.h")).read()
    assert "face_align.hip" in build.SOURCES and _lib.ABI_VERSION == 5
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in declared:
        assert hasattr(lib, name), name
        # the declaration's parameter list against the bound signature: pointers -> pointer types, integers in order
        decl = re.search(r"(int64_t|int) %s\(([^)]*)\)" % name, src)
        res, args = _lib._ALIGN_SIGS[name]
        assert res is (ctypes.c_int64 if decl.group(1) == "int64_t" else ctypes.c_int)
        kinds = []
        for arg in decl.group(2).split(","):
            if "double*" in arg:
                kinds.append("p" if name != "vt_align_quad" else "d")
            elif "*" in arg or "vt_stream" in arg:
                kinds.append("p")
            else:
                kinds.append("q" if "int64_t" in arg else "i")
        bound = ["d" if t is ctypes.POINTER(ctypes.c_double) else "p" if t is ctypes.c_void_p else "q" if t is ctypes.c_int64
                 else "i" for t in args]
        assert bound == kinds, (name, bound, kinds)
    assert re.search(r"align_all_parallel\.py:\d+", src)
