"""Cases of the face-alignment tests (tests/test_face_align.py, tests/test_align_cli.py) and of their fixture
(tests/golden/make_golden_align.py -> tests/golden/align.npz).  Plain module: no test functions.

An image is an integer formula of (y, x, c) and a seed -- regenerated identically everywhere, so the fixture holds only a
CRC32 of it -- and the 68 landmarks are built from the eye centre, the eye distance and the tilt of the face.  With the mouth
1.1 eye distances below the eyes the oriented crop rectangle has a side of 4 eye distances.
"""
import zlib

import numpy as np


def image(H, W, seed):
    y, x, c = np.ogrid[:H, :W, :3]
    y, x, c = y.astype(np.int64), x.astype(np.int64), c.astype(np.int64)
    grad = 2 * y + 3 * x + 70 * c + 11 * seed
    prod = ((y + 5 * seed) * (x + 3)) % 251
    hashy = (((y * 73856093) ^ (x * 19349663) ^ ((c + seed) * 83492791)) >> 5) % 97
    return ((grad + prod + hashy) % 256).astype(np.uint8)


def landmarks(centre, eye_distance, tilt):
    """(68,2) integer landmarks (dlib gives integers): eyes `eye_distance` apart around `centre` (x, y) on a line tilted by
    `tilt` radians, mouth corners 1.1 eye distances below; the other points are filled in but not read by the alignment."""
    cx, cy = centre
    ux, uy = np.cos(tilt), np.sin(tilt)                # along the eyes
    vx, vy = -uy, ux                                   # down the face
    d = float(eye_distance)
    lm = np.zeros((68, 2), dtype=np.float64)
    lm[:] = (cx + 0.4 * d * vx, cy + 0.4 * d * vy)
    ring = np.array([[-0.15, 0.0], [-0.07, -0.05], [0.07, -0.05], [0.15, 0.0], [0.07, 0.05], [-0.07, 0.05]]) * d
    for first, side in ((36, -0.5), (42, 0.5)):
        ex, ey = cx + side * d * ux, cy + side * d * uy
        lm[first:first + 6, 0] = ex + ring[:, 0] * ux + ring[:, 1] * vx
        lm[first:first + 6, 1] = ey + ring[:, 0] * uy + ring[:, 1] * vy
    mx, my = cx + 1.1 * d * vx, cy + 1.1 * d * vy
    lm[48] = (mx - 0.35 * d * ux, my - 0.35 * d * uy)
    lm[54] = (mx + 0.35 * d * ux, my + 0.35 * d * uy)
    return np.rint(lm).astype(np.int64)


# name -> (H, W, seed, eye centre (x, y), eye distance, tilt, branches the plan must take: shrink, crops, pads)
CASES = {
    "inside":   (360, 480, 1, (240, 150), 50, 0.1, (0, True, False)),      # a strict sub-rectangle, no pad
    "tiny":     (64, 80, 2, (40, 27), 12, 0.0, (0, True, False)),          # 64x80 image, eye distance 12, no pad
    "left":     (320, 400, 3, (50, 140), 40, -0.2, (0, True, True)),       # pad on the left larger than the others
    "corner":   (300, 300, 4, (250, 50), 40, 0.15, (0, True, True)),       # top-right corner: two different pads
    "whole":    (90, 100, 5, (50, 33), 28, 0.05, (0, False, True)),        # the image is smaller than the quad: pad all round
    "shrink2":  (560, 640, 6, (320, 220), 260, 0.05, (2, False, True)),    # 640x560 -> 320x280, with pad
    "shrink3":  (640, 768, 7, (384, 277), 385, -0.01, (3, False, True)),   # 768x640 -> 256x213 (rint), with pad: the pads
                                                                            # (just under 213) only fit a centred, upright face
}
NO_PAD = ("inside", "tiny")
PADDED = ("left", "corner", "whole", "shrink2", "shrink3")
# plan only: the pad would reach the side of the 60x60 image it reflects
TOO_LARGE = (60, 60, (30, 20), 40, 0.0)


def lm_of(name):
    return landmarks(*CASES[name][3:6])


def case(name):
    H, W, seed = CASES[name][:3]
    return image(H, W, seed), lm_of(name)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def check_branches(plan_of):
    """Each case takes the branches it was written for; `plan_of(lm, shape)` is the plan under test."""
    for name, (H, W, _, centre, d, tilt, (shrink, crops, pads)) in CASES.items():
        p = plan_of(landmarks(centre, d, tilt), (H, W))
        assert (p.shrink if p.shrink > 1 else 0) == shrink, (name, p.shrink)
        assert (p.crop is not None) == crops and (p.pad is not None) == pads, (name, p.crop, p.pad)
    p = plan_of(lm_of("left"), CASES["left"][:2])
    assert p.pad[0] > max(p.pad[1:]), p.pad
    p = plan_of(lm_of("corner"), CASES["corner"][:2])
    assert len(set(p.pad)) >= 2, p.pad
    assert plan_of(lm_of("shrink2"), CASES["shrink2"][:2]).rsize == (320, 280)
    assert plan_of(lm_of("shrink3"), CASES["shrink3"][:2]).rsize == (256, 213)
