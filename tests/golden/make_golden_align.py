#!/usr/bin/env python3
"""Golden fixture for the face alignment from the REAL reference (authoring container only; needs Pillow and scipy).

    python tests/golden/make_golden_align.py     # writes tests/golden/align.npz

model/encoder/align_all_parallel.py imports dlib, which is absent here: a stub module stands in, `get_landmark` is replaced by
a function that returns the case's landmarks (tests/align_cases.py), and the reference's OWN align_face runs on every case.
Pillow >= 10 has no Image.ANTIALIAS: it is aliased to LANCZOS, the same filter under its present name.  The plan numbers
(shrink, crop, pad, final quad) are captured by executing the same source lines (:69-142), read from the reference at run
time, in a namespace that is inspected afterwards.  Nothing is copied from the reference: only arrays it computes.
"""
import importlib.util
import json
import os
import sys
import textwrap
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VTOONIFY_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import PIL  # noqa: E402
import PIL.Image  # noqa: E402
import scipy  # noqa: E402
import scipy.ndimage  # noqa: E402

import align_cases as AC  # noqa: E402

if "dlib" not in sys.modules:
    sys.modules["dlib"] = types.ModuleType("dlib")
if not hasattr(PIL.Image, "ANTIALIAS"):
    PIL.Image.ANTIALIAS = PIL.Image.LANCZOS
SRC = os.path.join(REF, "model", "encoder", "align_all_parallel.py")
spec = importlib.util.spec_from_file_location("ref_align_all_parallel", SRC)
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)


def lines(a, b):
    with open(SRC) as f:
        return textwrap.dedent("".join(f.readlines()[a - 1:b]))


PLAN = compile(lines(69, 142), SRC, "exec")          # lm_chin = lm[0: 17] ... quad += pad[:2]
TRANSFORM = compile(lines(145, 145), SRC, "exec")


def main():
    out = {}
    for name in AC.CASES:
        img, lm = AC.case(name)
        ref.get_landmark = lambda filepath, predictor, lm=lm: lm
        got = np.asarray(ref.align_face(img, None))
        assert got.shape == (256, 256, 3) and got.dtype == np.uint8
        ns = {"np": np, "PIL": PIL, "scipy": scipy, "lm": lm, "filepath": img}
        exec(PLAN, ns)
        shrink, crop, pad = ns["shrink"], ns["crop"], ns["pad"]
        final = ns["img"]
        cropped = crop[2] - crop[0] < (ns["rsize"][0] if shrink > 1 else img.shape[1]) or \
            crop[3] - crop[1] < (ns["rsize"][1] if shrink > 1 else img.shape[0])
        padded = isinstance(pad, np.ndarray)            # np.maximum made it an array inside the branch
        exec(TRANSFORM, ns)
        assert np.array_equal(np.asarray(ns["img"]), got), name       # the traced lines are the function's
        out[f"{name}__out"] = got
        out[f"{name}__plan"] = np.array([shrink, *(ns["rsize"] if shrink > 1 else (0, 0)), int(cropped), *crop, int(padded),
                                         *[int(p) for p in pad], final.size[1], final.size[0]], dtype=np.int64)
        out[f"{name}__quad"] = np.asarray(ns["quad"], dtype=np.float64)
        out[f"{name}__crc"] = np.array([AC.crc(img), AC.crc(lm)], dtype=np.int64)
        print(name, img.shape, out[f"{name}__plan"].tolist())
    meta = {"pillow": PIL.__version__, "scipy": scipy.__version__, "numpy": np.__version__,
            "plan": "shrink, rsize W H, cropped, crop x0 y0 x1 y1, padded, pad l t r b, final h w"}
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "align.npz")
    np.savez_compressed(path, **out)
    print(f"wrote align.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
