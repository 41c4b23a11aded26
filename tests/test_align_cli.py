"""tools/style_transfer_amd.py --landmarks without dlib: the style encoder's input is the reference's aligned crop, made by
vtoonify_amd/align.py from the given landmarks (kernels on the engine, numpy with --cpu), not the squashed whole frame.

Host emulation and, under the gpu mark, the MI355X.  The pSp encoder is a stub that records its input; the frame loop is a
stub too (the frames are the business of tests/test_style_transfer_cli.py and tests/test_scale_cli.py), so a 360 x 480 clip
costs nothing in emulation.  The clip is two copies of the `inside` case of tests/align_cases.py, stored BGR.
"""
import os
import sys

import numpy as np
import pytest
import torch

import align_cases as AC
from conftest import REPO, load_golden
from vtoonify_amd import _lib, align as A, psp, scale as S

sys.path.insert(0, os.path.join(REPO, "tools"))
import style_transfer_amd as cli  # noqa: E402

GOLD, _ = load_golden("align.npz")
MESSAGE = "un-aligned first frame"


class _Encoder:
    """Stands in for vtoonify_amd.psp.GradualStyleEncoder: records what it is given, returns zeros (1,18,512)."""
    seen = []

    def __init__(self, *a, **k):
        pass

    def load_state_dict(self, sd):
        return self

    def eval(self):
        return self

    def to(self, device):
        return self

    def __call__(self, t):
        _Encoder.seen.append(t.detach().cpu().clone())
        return torch.zeros((1, 18, 512), dtype=torch.float32, device=t.device)


class _Loop:
    def __init__(self, *a, **k):
        pass

    def run(self, source, emit, first_index=0):
        return 0


@pytest.fixture
def clip(tmp_path, monkeypatch):
    img, lm = AC.case("inside")
    np.save(tmp_path / "clip.npy", np.stack([img[..., ::-1]] * 2, 0))
    np.save(tmp_path / "lm.npy", lm)
    np.save(tmp_path / "maps.npy", np.zeros((2, 19, 8, 8), dtype=np.float32))
    monkeypatch.setitem(sys.modules, "dlib", None)              # `import dlib` raises ImportError
    monkeypatch.setitem(sys.modules, "cv2", None)
    monkeypatch.setattr(psp, "GradualStyleEncoder", _Encoder)
    monkeypatch.setattr(cli, "VideoToonifier", _Loop)
    monkeypatch.setattr(cli, "_cpu_loop", lambda *a, **k: 0)
    _Encoder.seen = []
    return img, lm


def _args(tmp_path, *extra, landmarks=True):
    lm = ["--landmarks", str(tmp_path / "lm.npy")] if landmarks else []
    return ["--content", str(tmp_path / "clip.npy"), "--video", "--parsing_map_path", str(tmp_path / "maps.npy"),
            "--ckpt", "synthetic", "--style_encoder_path", "synthetic", "--backbone", "toonify", "--output_path",
            str(tmp_path / "out"), "--batch_size", "2", "--precision", "bf16", *lm, *extra]


def _normalised(u8):
    t = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1)[None].to(torch.float32)
    return ((t / 255.0) - 0.5) / 0.5


def test_landmarks_feed_the_aligned_crop_to_the_style_encoder(dev, clip, tmp_path, capsys):
    img, lm = clip
    cli.main(_args(tmp_path), device=str(dev))
    out = capsys.readouterr().out
    assert len(_Encoder.seen) == 1 and MESSAGE not in out
    assert torch.equal(_Encoder.seen[0], _normalised(GOLD["inside__out"]))           # the reference's crop, bit for bit

    # --scale_image: the crop is aligned on the scaled first frame, from the landmarks mapped onto it
    cli.main(_args(tmp_path, "--scale_image"), device=str(dev))
    out = capsys.readouterr().out
    assert len(_Encoder.seen) == 2 and MESSAGE not in out
    p = S.crop_parameters(lm, img.shape[:2], [200, 200, 200, 200])
    first = S.ScaleCrop(p, img.shape[0], img.shape[1]).host(img[..., ::-1])
    assert first.shape[0] < 461 and first.shape[1] < 614
    mapped = lm.astype(np.float64) * p.scale - (p.left, p.top)
    u8, x = A.FaceAligner(dev)(np.ascontiguousarray(first[..., ::-1]), mapped)
    assert torch.equal(_Encoder.seen[1], x.cpu())
    assert np.array_equal(u8.cpu().numpy(), A.align_face_host(np.ascontiguousarray(first[..., ::-1]), mapped))

    # without --landmarks: today's fallback and its message
    cli.main(_args(tmp_path, landmarks=False), device=str(dev))
    out = capsys.readouterr().out
    assert len(_Encoder.seen) == 3 and MESSAGE in out
    t = torch.from_numpy(img.copy()).to(dev).permute(2, 0, 1)[None].float() / 255.0
    t = torch.nn.functional.interpolate((t - 0.5) / 0.5, size=(256, 256), mode="bilinear", align_corners=False)
    assert torch.equal(_Encoder.seen[2], t.cpu())

    # --intrinsic_code still bypasses all of it
    np.save(tmp_path / "code.npy", np.zeros((1, 18, 512), dtype=np.float32))
    cli.main(_args(tmp_path, "--intrinsic_code", str(tmp_path / "code.npy")), device=str(dev))
    assert len(_Encoder.seen) == 3 and MESSAGE not in capsys.readouterr().out


def test_cpu_flag_takes_the_host_form(clip, tmp_path, capsys, monkeypatch):
    _lib.release_library()
    calls = []
    host = A.align_face_host
    monkeypatch.setattr(A, "align_face_host", lambda frame, lm: (calls.append(frame.shape), host(frame, lm))[1])
    cli.main(_args(tmp_path, "--cpu"))
    assert _lib._lib is None, "--cpu must not load a library"
    assert calls == [(360, 480, 3)] and len(_Encoder.seen) == 1 and MESSAGE not in capsys.readouterr().out
    assert torch.equal(_Encoder.seen[0], _normalised(GOLD["inside__out"]))


def test_style_input_is_a_function_of_its_own(dev, clip):
    """style_input, called directly: (1,3,256,256) float32 on the device, from an RGB frame as well."""
    img, lm = clip
    logged = []
    x = cli.style_input(cli.parse([]), img, False, torch.device(dev), logged.append, lm)
    assert x.device.type == torch.device(dev).type and x.dtype == torch.float32 and not logged
    assert torch.equal(x.cpu(), _normalised(GOLD["inside__out"]))
    y = cli.style_input(cli.parse([]), img, False, torch.device(dev), logged.append)
    assert tuple(y.shape) == (1, 3, 256, 256) and len(logged) == 1 and MESSAGE in logged[0]
