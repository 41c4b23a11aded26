"""tools/generate_amd.py on synthetic weights at --size 64: the written array equals the module chain
(face -> alignment from --landmarks -> pSp -> zplus2wplus -> DualStyleGAN.forward, and the sampled Generator), the same --seed
gives the same bytes, the extrinsic style is taken in the key order of the dict in exstyle_code.npy.

The CPU suite runs the plain torch executor (device "cpu", no emulation: a size-64 model takes minutes as coroutines) with a
stub for the pSp encoder, which has no CPU path; -m gpu runs the whole chain on the MI355X with the real synthetic encoder.
The face is the `inside` case of tests/align_cases.py, aligned without dlib.
"""
import os
import sys

import numpy as np
import pytest
import torch

import align_cases as AC
from conftest import REPO, load_golden
from vtoonify_amd import _lib, align as A, psp, synth

sys.path.insert(0, os.path.join(REPO, "tools"))
import generate_amd  # noqa: E402

GOLD, _ = load_golden("align.npz")


class _Encoder:
    """Stands in for vtoonify_amd.psp.GradualStyleEncoder on the CPU: a z+ code that is a fixed function of its input."""

    def __init__(self, *a, **k):
        pass

    def load_state_dict(self, sd):
        return self

    def eval(self):
        return self

    def to(self, device):
        return self

    def __call__(self, t):
        rows = torch.nn.functional.adaptive_avg_pool2d(t[:, :1], (18, 512))[:, 0]
        return rows * 3.0 + torch.linspace(-1, 1, 18 * 512).reshape(1, 18, 512)


def _bind(target, monkeypatch):
    monkeypatch.setitem(sys.modules, "dlib", None)              # `import dlib` raises ImportError: alignment from --landmarks
    if target == "cpu":
        _lib.release_library()
        monkeypatch.setattr(psp, "GradualStyleEncoder", _Encoder)
        return torch.device("cpu")
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    _lib.use_library(_lib.DEFAULT_LIB)
    return torch.device("cuda:0")


@pytest.mark.parametrize("target", ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_generate_cli_portrait(target, tmp_path, monkeypatch):
    device = _bind(target, monkeypatch)
    img, lm = AC.case("inside")
    np.save(tmp_path / "face.npy", img)
    np.save(tmp_path / "lm.npy", lm)
    # the reference's dict form, NOT stored in sorted order: --style_id counts keys as they were inserted
    codes = {name: torch.randn(1, 18, 512, generator=torch.Generator().manual_seed(i)).numpy()
             for i, name in enumerate(["zebra.jpg", "apple.jpg", "mango.jpg"])}
    np.save(tmp_path / "exstyle_code.npy", codes, allow_pickle=True)
    weight = [str(0.25 + 0.04 * i) for i in range(18)]
    argv = ["--ckpt", "synthetic", "--style_encoder_path", "synthetic", "--size", "64", "--seed", "3", "--content",
            str(tmp_path / "face.npy"), "--landmarks", str(tmp_path / "lm.npy"), "--exstyle_path", str(tmp_path / "exstyle_code.npy"),
            "--style_id", "1", "--weight", *weight, "--output_path", str(tmp_path / "a")]
    a = generate_amd.main(argv, device=device)
    saved = np.load(a["path"])
    assert saved.shape == (1, 3, 64, 64) and saved.dtype == np.float32 and np.isfinite(saved).all()

    # the module chain, written out
    opt = generate_amd.parse(argv)
    model = generate_amd.load_model(opt, device)
    if target == "cpu":
        x = torch.from_numpy(A.normalise_host(A.align_face_host(img, lm)))
        enc = _Encoder()
    else:
        x = A.FaceAligner(device)(img, lm)[1]
        enc = psp.GradualStyleEncoder(50, "ir_se", compute_dtype=torch.float32)
        enc.load_state_dict(synth.synth_state_dict(generate_amd_shapes("psp"), 3))
        enc = enc.eval().to(device)
    u8 = np.clip(np.rint((x[0].cpu().numpy().transpose(1, 2, 0) * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8)
    assert np.array_equal(u8, GOLD["inside__out"]), "the encoder sees the reference's aligned crop"
    with torch.no_grad():
        z = enc(x.to(device)).float()[:, :model.n_latent].contiguous()
        ex = torch.from_numpy(codes["apple.jpg"]).to(device)[:, :model.n_latent].contiguous()
        w = model.get_latent(z.reshape(-1, 512)).reshape(z.shape)
        exw = model.get_latent(ex.reshape(-1, 512)).reshape(ex.shape)
        torch.manual_seed(3)
        want, _ = model([w], exw, input_is_latent=True, interp_weights=[float(v) for v in weight])
    assert np.array_equal(saved, want.float().cpu().numpy()), "the written array equals the module chain"

    b = generate_amd.main(argv[:-1] + [str(tmp_path / "b")], device=device)
    assert open(a["path"], "rb").read() == open(b["path"], "rb").read(), "the same --seed gives the same bytes"
    c = generate_amd.main(argv[:-1] + [str(tmp_path / "c"), "--style_id", "0"], device=device)
    assert not np.array_equal(np.load(c["path"]), saved), "another style"
    # --intrinsic_code is a z+ code, as in tools/style_transfer_amd.py: the same chain without the encoder
    np.save(tmp_path / "zplus.npy", enc(x.to(device)).float().cpu().numpy())
    i = argv.index("--content")
    d = generate_amd.main(argv[:i] + argv[i + 4:-1] + [str(tmp_path / "d"), "--intrinsic_code", str(tmp_path / "zplus.npy")],
                          device=device)
    assert np.array_equal(np.load(d["path"]), saved)


def generate_amd_shapes(tag):
    from style_transfer_amd import _shapes
    return _shapes(tag)


@pytest.mark.parametrize("target", ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_generate_cli_samples_the_generator(target, tmp_path, monkeypatch):
    device = _bind(target, monkeypatch)
    argv = ["--ckpt", "synthetic", "--size", "64", "--seed", "3", "--truncation", "0.7", "--output_path", str(tmp_path / "a")]
    a = generate_amd.main(argv, device=device)
    saved = np.load(a["path"])
    assert saved.shape == (1, 3, 64, 64) and np.isfinite(saved).all()
    model = generate_amd.load_model(generate_amd.parse(argv), device)
    torch.manual_seed(3)
    mean = model.mean_latent(4096)
    want, _ = model.generator([torch.randn(1, 512).to(device)], truncation=0.7, truncation_latent=mean)
    assert np.array_equal(saved, want.float().cpu().numpy())
    b = generate_amd.main(argv[:-1] + [str(tmp_path / "b")], device=device)
    assert open(a["path"], "rb").read() == open(b["path"], "rb").read()
    c = generate_amd.main(argv[:-1] + [str(tmp_path / "c"), "--seed", "4"], device=device)
    assert not np.array_equal(np.load(c["path"]), saved)
