#!/usr/bin/env python3
"""Golden fixture for the whole flicker-reduction pre-pass from the REAL reference (authoring container only).

    python tests/golden/make_golden_smooth_stream.py     # writes tests/golden/smooth_stream{,_b,_c}.npz

smooth_parsing_map.py cannot be imported here (cv2 / torchvision / tqdm are absent, `warp` calls .cuda()), so this script
EXECUTES the reference's own source lines, read from the reference checkout at run time, on the CPU: the `warp` function
(:37-75), the up-sampling and end replication (:128-129), the parsing loop (:133-138), the temporal weights (:144) and
the main loop (:146-167) -- with `Tensor.cuda` a no-op, device = "cpu", tqdm the identity, and the reference's own RAFT,
InputPadder, BiSeNet and Downsample classes.  Both networks carry the synthetic weights of vtoonify_amd.synth (seed 0,
their schemas are tests/golden/keys_raft.json / keys_bisenet.json).  `transform` (:86-89) is restated as the two
torchvision formulas, ToTensor = HWC uint8 -> CHW float / 255 and Normalize = (x - 0.5) / 0.5.  Nothing is copied from
the reference: only tensors it computes.

The clip: 7 RGB frames of 64 x 64 uint8 (128 x 128 after the doubling, a multiple of 8), window 2 -- a smooth pattern
that drifts by a little over one pixel per frame.
"""
import argparse
import importlib
import os
import sys
import textwrap
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VTOONIFY_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import torch.utils.model_zoo as modelzoo  # noqa: E402
from torch import nn  # noqa: E402

_cpu = importlib.import_module("model.stylegan.op_cpu")
_gf = importlib.import_module("model.stylegan.op_cpu.conv2d_gradfix")
sys.modules["model.stylegan.op"] = _cpu
sys.modules["model.stylegan.op.conv2d_gradfix"] = _gf
_cpu.conv2d_gradfix = _gf
sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
modelzoo.load_url = lambda *a, **k: {}
from model.bisenet.model import BiSeNet  # noqa: E402
from model.raft.core.raft import RAFT  # noqa: E402
from model.raft.core.utils.utils import InputPadder  # noqa: E402
from model.stylegan.model import Downsample  # noqa: E402

sys.path.append(REPO)
from vtoonify_amd import synth  # noqa: E402

torch.set_grad_enabled(False)
torch.Tensor.cuda = lambda self, *a, **k: self
SRC = os.path.join(REF, "smooth_parsing_map.py")
T, H, W, WINDOW = 7, 64, 64, 2


def lines(a, b):
    with open(SRC) as f:
        return textwrap.dedent("".join(f.readlines()[a - 1:b]))


def make_clip():
    """A smooth texture (sum of a few sinusoids per channel + a soft blob) translating (1.3, 0.7) pixels per frame."""
    g = np.random.default_rng(17)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    waves = [(g.uniform(0.05, 0.35, 2), g.uniform(0, 2 * np.pi), c) for c in range(3) for _ in range(4)]
    frames = np.zeros((T, H, W, 3), np.uint8)
    for t in range(T):
        x, y = xx - 1.3 * t, yy - 0.7 * t
        img = np.zeros((H, W, 3))
        for (fx, fy), ph, c in waves:
            img[..., c] += np.sin(fx * x + fy * y + ph)
        blob = np.exp(-((x - 24) ** 2 + (y - 30) ** 2) / (2 * 9.0 ** 2))
        img = img / 4 * 0.6 + blob[..., None] * np.array([0.9, -0.5, 0.4])
        frames[t] = np.clip(np.round((img * 0.5 + 0.5) * 255), 0, 255).astype(np.uint8)
    return frames


def main():
    frames = make_clip()
    raft_model = RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).eval()
    raft_model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in raft_model.state_dict().items()}, 0))
    parsingpredictor = BiSeNet(n_classes=19).eval()
    parsingpredictor.load_state_dict(
        synth.synth_state_dict({k: tuple(v.shape) for k, v in parsingpredictor.state_dict().items()}, 0))
    ns = {"torch": torch, "nn": nn}
    exec(compile(lines(37, 75), SRC, "exec"), ns)       # def warp(x, flo)
    transform = lambda fr: (torch.from_numpy(fr).permute(2, 0, 1).contiguous().float().div(255) - 0.5) / 0.5
    env = {"torch": torch, "F": F, "np": np, "warp": ns["warp"], "tqdm": lambda it: it, "device": "cpu",
           "window": WINDOW, "InputPadder": InputPadder, "raft_model": raft_model, "parsingpredictor": parsingpredictor,
           "down": Downsample(kernel=[1, 3, 3, 1], factor=2).eval(),
           "Is": [transform(fr).unsqueeze(dim=0).cpu() for fr in frames]}        # :124
    for a, b in ((128, 129), (133, 138), (144, 144), (146, 167)):
        exec(compile(lines(a, b), SRC, "exec"), env)
    parse = env["parse"].numpy()
    assert parse.shape == (T, 19, H, W) and np.isfinite(parse).all()
    print("parse", parse.shape, "max|parse|", float(np.abs(parse).max()), "max|Ps|", float(env["Ps"].abs().max()))
    # parse is 2.2 MB of fp32: three files, each under the size limit of a committed fixture
    parts = {"smooth_stream.npz": {"frames": frames, "parse_0_2": parse[0:2],
                                   "cfg": np.array([WINDOW, 20, 0, 0])},   # window, RAFT iterations, synth seeds
             "smooth_stream_b.npz": {"parse_2_5": parse[2:5]}, "smooth_stream_c.npz": {"parse_5_7": parse[5:7]}}
    for name, d in parts.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **d)
        print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
