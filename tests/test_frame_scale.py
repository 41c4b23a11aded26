"""--scale_image on the GPU: vt_frame_scale_crop (csrc/frame_scale.hip), vtoonify_amd/scale.py and the video driver's
`prescale`, in host emulation (CPU suite) and on the MI355X (-m gpu).

The reference of the kernel is the restatement below: the integer arithmetic of DESIGN.md 4.8 written out in plain
numpy / int64 from the formulas, independent of vtoonify_amd/scale.py (np.pad's 'reflect' IS reflect-101; the tables are built
one element at a time with float32 scalars).  uint8 / integer work: every comparison is BIT-exact.

Tile sizes of the kernel: 32x32, 16x16, 8x8 (the launcher takes the largest whose source footprint fits its LDS).  Output
20x28 is 2x2 tiles of 8 and of 16 plus a ragged edge both ways (the 16-tile is what scale 0.3 with two passes gets on the
97x131 source); 40x44 is the same for the 32-tile where the resized frame is large enough to hold it; 8x8 is one tile.
"""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from conftest import REPO, load_keys
from vtoonify_amd import _lib, scale as S, synth, video
from vtoonify_amd.engine import VToonifyEngine

TAPS = (32, 96, 96, 32)
SENTINEL, GUARD = 0xA5, 64


# ------------------------------------------------------------------------------------------- the restatement
def passes_for(scale):
    return 0 if scale > 0.75 else 1 if scale > 0.375 else 2


def ref_axis(lo, hi, dst, src, horizontal):
    sc = 1.0 / (dst / src)
    tab = []
    for d in range(lo, hi):
        f = np.float32((d + 0.5) * sc - 0.5)
        i = int(np.floor(f))
        f = np.float32(f - np.float32(i))
        if horizontal:
            if i < 0:
                i, f = 0, np.float32(0)
            if i >= src - 1:
                i, f = src - 1, np.float32(0)
            i0, i1 = i, min(i + 1, src - 1)
        else:
            i0, i1 = min(max(i, 0), src - 1), min(max(i + 1, 0), src - 1)
        w0 = int(np.rint(np.float32(np.float32(1) - f) * np.float32(2048)))
        w1 = int(np.rint(f * np.float32(2048)))
        tab.append((i0, i1, w0, w1))
    return np.array(tab, dtype=np.int32).reshape(-1, 4)


def ref_blur(P):
    Pp = np.pad(P.astype(np.int64), ((2, 1), (2, 1), (0, 0)), mode="reflect")      # r(-1) = 1, r(n) = n-2
    Hs, Ws = P.shape[:2]
    acc = np.zeros(P.shape, dtype=np.int64)
    for i in range(4):
        for j in range(4):
            acc += TAPS[i] * TAPS[j] * Pp[i:i + Hs, j:j + Ws]
    return ((acc + 32768) >> 16).astype(np.uint8)


def ref_crop(frame, passes, xtab, ytab):
    Q = frame
    for _ in range(passes):
        Q = ref_blur(Q)
    Q = Q.astype(np.int64)
    out = np.zeros((len(ytab), len(xtab), 3), dtype=np.int64)
    for oy, (y0, y1, b0, b1) in enumerate(ytab.astype(np.int64)):
        for ox, (x0, x1, a0, a1) in enumerate(xtab.astype(np.int64)):
            h0 = a0 * Q[y0, x0] + a1 * Q[y0, x1]
            h1 = a0 * Q[y1, x0] + a1 * Q[y1, x1]
            out[oy, ox] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def ref_rows(ytab, passes, Hs):
    """Source rows the crop and its blur halo read: (row0, rows)."""
    need = set(int(v) for v in ytab[:, :2].reshape(-1))
    need = set(range(min(need), max(need) + 1))
    refl = lambda i: -i if i < 0 else 2 * (Hs - 1) - i if i >= Hs else i
    for _ in range(passes):
        need = {refl(y + o) for y in need for o in (-2, -1, 0, 1)}
    return min(need), max(need) - min(need) + 1


def window(scale, Hs, Ws, H, W, where):
    h, w = round(Hs * scale), round(Ws * scale)
    assert H <= h and W <= w
    top, left = {"tl": (0, 0), "br": (h - H, w - W), "mid": ((h - H) // 2, (w - W) // 2)}[where]
    return ref_axis(left, left + W, w, Ws, True), ref_axis(top, top + H, h, Hs, False), (h, w, top, left)


# ------------------------------------------------------------------------------------------------- 1. the kernel, bit-exact
def _launch(dev, src, n, rows, row0, Hs, Ws, passes, xtab, ytab, H, W):
    """vt_frame_scale_crop into a buffer with 64 guard bytes of a sentinel either side -> (rc, out (n,H,W,3), guards intact)."""
    m = max(n, 1)                                                    # (n = 0 is one of the refused calls)
    buf = torch.full((m * H * W * 3 + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    d_src = torch.from_numpy(np.array(src)).to(dev)              # (a copy: the shared sources are read-only)
    xt, yt = torch.from_numpy(np.ascontiguousarray(xtab)).to(dev), torch.from_numpy(np.ascontiguousarray(ytab)).to(dev)
    rc = _lib.lib().vt_frame_scale_crop(buf.data_ptr() + GUARD, d_src.data_ptr(), n, rows, row0, Hs, Ws, passes, xt.data_ptr(),
                                        yt.data_ptr(), H, W, video._stream(d_src))
    b = buf.cpu().numpy()
    intact = bool((b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all())
    return rc, b[GUARD:-GUARD].reshape(m, H, W, 3), intact


_SRC = {}


def _source(Hs, Ws, n=3):
    if (Hs, Ws) not in _SRC:
        f = np.random.default_rng(Hs * 1000 + Ws).integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)
        f[0, 0, 0], f[-1, -1, -1] = 0, 255
        f.setflags(write=False)
        _SRC[(Hs, Ws)] = f
    return _SRC[(Hs, Ws)]


def _check(dev, frames, scale, H, W, where, passes=None):
    n, Hs, Ws, _ = frames.shape
    passes = passes_for(scale) if passes is None else passes
    xtab, ytab, _ = window(scale, Hs, Ws, H, W, where)
    want = np.stack([ref_crop(f, passes, xtab, ytab) for f in frames], 0)
    row0, rows = ref_rows(ytab, passes, Hs)
    for r0, nr in ((row0, rows), (0, Hs)):                        # the slab the crop needs, and the whole frame
        rc, got, intact = _launch(dev, frames[:, r0:r0 + nr], n, nr, r0, Hs, Ws, passes, xtab, ytab, H, W)
        assert rc == 0, _lib.lib().vt_last_error().decode()
        assert intact, "guard bytes overwritten"
        bad = np.argwhere(got != want)
        assert bad.size == 0, (scale, where, (H, W), (r0, nr), len(bad), bad[:4].tolist())
    return row0, rows


def _cases():
    out = []
    for scale in (1.6, 0.9, 0.6, 0.3):
        for where in ("tl", "br", "mid"):
            sizes = [(20, 28), (8, 8)] + ([(40, 44)] if scale >= 0.6 else [])
            out += [(scale, where, hw) for hw in sizes]
    return out


@pytest.mark.parametrize("scale,where,hw", _cases())
def test_frame_scale_crop_bit_exact(dev, scale, where, hw):
    """vt_frame_scale_crop against the restatement: four scales (0, 0, 1 and 2 blur passes), windows at the top-left corner,
    at the bottom-right corner (x1 / y1 clamp, reflect-101 on the high side) and inside, slab and whole-frame form."""
    row0, rows = _check(dev, _source(97, 131), scale, hw[0], hw[1], where)
    if where == "br" and hw == (8, 8):
        assert row0 > 0 and row0 + rows == 97          # the slab form really is a slab


def test_frame_scale_crop_small_tile_and_odd_width(dev):
    """Scale 0.2 on a 200x260 source: two passes over ~5 source pixels per output pixel, only the 8x8 tile fits the LDS.  An
    output width that is no multiple of 4 (rows start at any byte: the byte-store path), at every pass count."""
    big = _source(200, 260, n=2)
    _check(dev, big, 0.2, 24, 32, "mid")
    _check(dev, big, 0.2, 40, 52, "tl")                 # the whole resized frame: both borders at once
    for scale in (1.6, 0.6, 0.3):
        _check(dev, _source(97, 131), scale, 9, 13, "br")
    # two passes asked of an up-scaling table (the ABI does not tie `passes` to the scale): footprint smaller than the halo
    _check(dev, _source(97, 131), 1.6, 20, 28, "tl", passes=2)
    # scale 1/8 (eye distance 512), two passes: the limit the launcher must still serve
    _check(dev, _source(200, 260, n=2), 0.125, 16, 24, "br")


# ----------------------------------------------------------------------------------------------- 2. tables and parameters
def _params(scale, Hs, Ws, top, left, H, W):
    return S.CropParams(scale, round(Hs * scale), round(Ws * scale), left, left + W, top, top + H, passes_for(scale))


@pytest.mark.parametrize("scale", [1.6, 0.9, 0.6, 0.3])
def test_scalecrop_tables_equal_the_restatement(scale):
    Hs, Ws = 97, 131
    h, w = round(Hs * scale), round(Ws * scale)
    if scale == 0.3:
        assert w == 39                                            # where float32 rounding of f matters
    sc = S.ScaleCrop(S.CropParams(scale, h, w, 0, w, 0, h, passes_for(scale)), Hs, Ws)     # every column and row
    xt, yt = ref_axis(0, w, w, Ws, True), ref_axis(0, h, h, Hs, False)
    assert sc.xtab.dtype == np.int32 and sc.xtab.shape == (w, 4) and np.array_equal(sc.xtab, xt)
    assert sc.ytab.dtype == np.int32 and sc.ytab.shape == (h, 4) and np.array_equal(sc.ytab, yt)
    assert (sc.row0, sc.rows) == ref_rows(yt, sc.passes, Hs) == (0, Hs)
    sub = S.ScaleCrop(_params(scale, Hs, Ws, h // 2, 8, 8, 16), Hs, Ws)
    assert np.array_equal(sub.xtab, xt[8:24]) and np.array_equal(sub.ytab, yt[h // 2:h // 2 + 8])
    assert (sub.row0, sub.rows) == ref_rows(sub.ytab, sub.passes, Hs) and sub.rows < Hs
    # the host form is the same arithmetic
    f = _source(Hs, Ws)[1]
    assert np.array_equal(sub.host(f), ref_crop(f, sub.passes, sub.xtab, sub.ytab))


def _landmarks(left_eye, right_eye):
    lm = np.zeros((68, 2))
    spread = np.array([[-10, -2], [-5, -1], [0, 0], [0, 0], [5, 1], [10, 2]], dtype=np.float64)
    lm[36:42] = np.array(left_eye) + spread
    lm[42:48] = np.array(right_eye) + spread
    return lm


# (landmarks, frame shape, padding) -> scale, h, w, left, right, top, bottom, passes; worked by hand:
#  a: eyes 128 apart -> scale 0.5, centre (164,120)*0.5 = (82,60); 480x640 -> 240x320; left 42//8*8, right 132//8*8,
#     top 30//8*8, bottom 130//8*8; 0.375 < 0.5 <= 0.75 -> one pass
#  b: eyes 200 apart -> scale 0.32, centre (400,250)*0.32 = (128,80); 720x1280 -> round(230.4) x round(409.6); padding runs
#     off the frame on every side: left max(-72,0), right min(428,410)//8*8, top max(-20,0), bottom min(280,230)//8*8; two passes
HAND = [
    (_landmarks((100, 120), (228, 120)), (480, 640), (40, 50, 30, 70), (0.5, 240, 320, 40, 128, 24, 128, 1)),
    (_landmarks((300, 250), (500, 250)), (720, 1280), (200, 300, 100, 200), (0.32, 230, 410, 0, 408, 0, 224, 2)),
]


@pytest.mark.parametrize("lm,shape,padding,want", HAND)
def test_crop_parameters_hand_computed_and_equal_facecrop(monkeypatch, lm, shape, padding, want):
    p = S.crop_parameters(lm, shape, padding)
    assert tuple(p) == want and all(type(v) is int for v in p[1:])
    assert S.crop_parameters(lm, shape + (3,), list(padding)) == p
    # ... and what the driver's FaceCrop.__init__ (the reference's formula, util.py:163-188) computes from the same landmarks
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import style_transfer_amd as cli
    monkeypatch.setitem(sys.modules, "cv2", types.ModuleType("cv2"))          # only imported by __init__, never called
    fc = cli.FaceCrop(np.zeros(shape + (3,), dtype=np.uint8), True, list(padding), landmarks=lm)
    assert (fc.scale, fc.h, fc.w, fc.left, fc.right, fc.top, fc.bottom) == tuple(p)[:7]
    assert (0 if fc.scale > 0.75 else 1 if fc.scale > 0.375 else 2) == p.passes          # FaceCrop.__call__'s two tests


# ------------------------------------------------------------------------------------------------- 3. errors, not faults
def test_inconsistent_arguments_are_errors_and_launch_nothing(dev):
    frames = _source(97, 131)
    n, Hs, Ws, _ = frames.shape
    H, W = 20, 28
    xtab, ytab, _ = window(0.6, Hs, Ws, H, W, "mid")
    row0, rows = ref_rows(ytab, 1, Hs)
    slab = frames[:, row0:row0 + rows]

    def refused(what, **kw):
        a = dict(src=slab, n=n, rows=rows, row0=row0, Hs=Hs, Ws=Ws, passes=1, xtab=xtab, ytab=ytab, H=H, W=W)
        a.update(kw)
        rc, got, intact = _launch(dev, a["src"], a["n"], a["rows"], a["row0"], a["Hs"], a["Ws"], a["passes"], a["xtab"],
                                  a["ytab"], a["H"], a["W"])
        msg = _lib.lib().vt_last_error().decode()
        assert rc != 0 and "vt_frame_scale_crop" in msg, (what, rc, msg)
        assert intact and (got == SENTINEL).all(), f"{what}: a kernel ran"
        return msg

    assert "slab" in refused("halo row missing above", src=slab[:, 1:], rows=rows - 1, row0=row0 + 1)
    assert "slab" in refused("halo row missing below", src=slab[:, :-1], rows=rows - 1)
    refused("slab runs past the frame", row0=Hs - rows + 1)
    bad = xtab.copy()
    bad[5, 1] = Ws
    assert "xtab[5]" in refused("x1 == Ws", xtab=bad)
    bad = ytab.copy()
    bad[3, 0] = -1
    assert "ytab[3]" in refused("y0 < 0", ytab=bad)
    bad = xtab.copy()
    bad[0, 2] = 4096
    refused("weight outside 0..2048", xtab=bad)
    assert "passes" in refused("passes = 3", passes=3)
    refused("n = 0", n=0)
    # below 1/8 the footprint of the smallest tile does not fit: an error that names the limit
    big = _source(200, 260, n=2)
    xt, yt, _ = window(0.05, 200, 260, 8, 8, "tl")
    rc, got, intact = _launch(dev, big, 2, 200, 0, 200, 260, 2, xt, yt, 8, 8)
    assert rc != 0 and "1/8" in _lib.lib().vt_last_error().decode() and (got == SENTINEL).all()
    # the adapter raises
    sc = S.ScaleCrop(_params(0.6, Hs, Ws, 8, 8, 16, 24), Hs, Ws).to(dev)
    with pytest.raises(_lib.VtError):
        sc.apply(torch.zeros((1, sc.rows + 1, Ws, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.VtError):
        sc.apply(torch.zeros((1, sc.rows, Ws, 3), dtype=torch.float32, device=dev))


def test_frames_header_binding_and_export():
    """include/vtoonify_amd_frames.h as tests/test_smooth_stream.py treats the pre-pass header: what it declares is what _lib
    binds (its own dict, not the list pinned to vtoonify_amd.h), the gfx950 library exports it, the main header includes it."""
    from vtoonify_amd import build
    src = open(os.path.join(REPO, "include", "vtoonify_amd_frames.h")).read()
    declared = sorted(set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.FRAMES_SYMBOLS) == ["vt_frame_scale_crop"]
    assert not set(declared) & set(_lib.EXPORTED_SYMBOLS) and not set(declared) & set(_lib.PREPASS_SYMBOLS)
    assert '#include "vtoonify_amd_frames.h"' in open(os.path.join(REPO, "include", "vtoonify_amd.h")).read()
    assert "frame_scale.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "vt_frame_scale_crop")
    # the declaration's parameter list against the bound signature: pointers -> c_void_p, int -> c_int, in order
    decl = re.search(r"int vt_frame_scale_crop\(([^)]*)\)", src).group(1)
    kinds = [ctypes.c_void_p if ("*" in a or "vt_stream" in a) else ctypes.c_int for a in decl.split(",")]
    res, args = _lib._FRAMES_SIGS["vt_frame_scale_crop"]
    assert res is ctypes.c_int and args == kinds and len(args) == 13
    block = src[:src.index("int vt_frame_scale_crop(")].rsplit("/*", 1)[1]
    assert block.rstrip().endswith("*/") and re.search(r"style_transfer\.py:\d+", block)


# --------------------------------------------------------------------------------------------------- 4. driver equivalence
def test_video_driver_prescale_equals_precropped_frames(dev):
    """VideoToonifier(prescale=sc) on 64x88 source frames == VideoToonifier() on the restatement's crops of the same frames, bit
    for bit; batch 2, depth 2, 5 frames (ragged last batch)."""
    n, Hs, Ws = 5, 64, 88
    g = np.random.default_rng(11)
    frames = g.integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)
    p = _params(0.6, Hs, Ws, 8, 16, 16, 24)
    parsing = (g.standard_normal((n, 19, 16, 24)) * 4).astype(np.float32)
    sd = synth.synth_state_dict(load_keys("T"), 0)
    eng = VToonifyEngine({k: v.to(dev) for k, v in sd.items()}, "toonify", 256, torch.bfloat16, dev)
    style = synth.synth_style(seed=5).to(dev)
    sc = S.ScaleCrop(p, Hs, Ws).to(dev)
    crops = np.stack([ref_crop(f, sc.passes, sc.xtab, sc.ytab) for f in frames], 0)
    assert np.array_equal(sc(frames[2]), crops[2]) and np.array_equal(sc.host(frames[2]), crops[2])   # one host frame

    def run(vt, fr):
        got, order = {}, []
        assert vt.run(((fr[i], parsing[i]) for i in range(n)), lambda i, o: (order.append(i), got.__setitem__(i, o.copy()))) == n
        assert order == list(range(n))
        return got

    plain = video.VideoToonifier(eng, style, None, batch_size=2, bgr=True, depth=2)
    want = run(plain, crops)
    assert all(s.d_src is None and tuple(s.h_frames.shape) == (2, 16, 24, 3) for s in plain._slots)      # prescale=None: as before
    pre = video.VideoToonifier(eng, style, None, batch_size=2, bgr=True, depth=2, prescale=sc)
    got = run(pre, frames)
    assert all(tuple(s.h_frames.shape) == (2, sc.rows, Ws, 3) for s in pre._slots) and sc.rows < Hs       # only the slab is staged
    for i in range(n):
        assert got[i].shape == (64, 96, 3) and np.array_equal(got[i], want[i]), i
    with pytest.raises(_lib.VtError):
        pre.run(iter([(crops[0], parsing[0])]), lambda i, o: None)            # a frame that is not source-size


# ------------------------------------------------------------------------------------------------------ 6. cv2, if there
def test_kernel_against_cv2(dev):
    """Only where cv2 is importable (it is not on the machines this suite was written on: the test then SKIPS and agreement with
    cv2 stays unverified).  cv2.sepFilter2D + cv2.resize + slice on the shapes of test 1: at most 1 count."""
    cv2 = pytest.importorskip("cv2", reason="cv2 not importable: agreement of the arithmetic with cv2 is unverified")
    k = np.array([[0.125], [0.375], [0.375], [0.125]])
    frames = _source(97, 131)
    worst = 0
    for scale, where, (H, W) in _cases():
        xtab, ytab, (h, w, top, left) = window(scale, 97, 131, H, W, where)
        passes = passes_for(scale)
        rc, got, _ = _launch(dev, frames, 3, 97, 0, 97, 131, passes, xtab, ytab, H, W)
        assert rc == 0
        for f, o in zip(frames, got):
            q = f
            for _ in range(passes):
                q = cv2.sepFilter2D(q, -1, k, k)
            ref = cv2.resize(q, (w, h))[top:top + H, left:left + W]
            worst = max(worst, int(np.abs(ref.astype(np.int32) - o.astype(np.int32)).max()))
    print(f"[cv2] max |kernel - cv2| = {worst} counts")
    assert worst <= 1
