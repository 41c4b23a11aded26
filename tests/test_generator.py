"""Generator.forward and DualStyleGAN.forward (vtoonify_amd/generator.py) against the reference's own modules
(tests/golden/generator*.npz from tests/golden/make_golden_generator.py; cases and inputs in tests/generator_cases.py).

  * the plain torch executor of modules on the CPU: every size-64 case within 1e-5 of max|golden|;
  * GeneratorEngine through the `dev` fixture: host emulation runs the size-32 model (size 64 takes minutes as coroutines),
    the MI355X the size-64 model and one 1024^2 case; fp32 (three-term bf16 products) and fp32_exact within 1e-4 of
    max|golden| -- the project's fp32 bar (README "Parity");
  * bf16 / fp16: no bar was known in advance.  The test prints max|d| / max|golden| and PSNR per case; the bars are twice the
    error measured on the MI355X (BARS below, profiles/generator_parity.txt);
  * noise through the engine, the module surface, and VToonify.forward unchanged by a generator call.
"""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import generator_cases as GC
from conftest import GOLDEN, load_golden, load_keys, psnr, rel_err
from vtoonify_amd import _lib, generator as G, synth
from vtoonify_amd.vtoonify import VToonify

GOLD = {64: load_golden("generator.npz")[0], 32: load_golden("generator_32.npz")[0]}
GOLD_FULL = load_golden("generator_1024.npz")[0]
CASES = list(GC.cases(64))
PRECISIONS = {"fp32": (torch.float32, False), "fp32_exact": (torch.float32, True), "bf16": (torch.bfloat16, False),
              "fp16": (torch.float16, False)}
# relative bound / PSNR floor per precision.  fp32: the project's 1e-4.  16-bit: twice the error measured on the MI355X over the
# size-64 cases (profiles/generator_parity.txt): bf16 worst 2.24e-2 / 52.3 dB, fp16 worst 2.38e-3 / 69.8 dB
# (twice the error = 6 dB less; both floors stay above the project's 45 dB)
BARS = {"fp32": (1e-4, None), "fp32_exact": (1e-4, None), "bf16": (4.5e-2, 46.0), "fp16": (4.8e-3, 63.0)}
_MODELS = {}


def _models(size, device, precision="fp32"):
    """One DualStyleGAN (and its inner Generator) per (size, device, precision), synthetic weights, shared by the tests."""
    key = (size, str(device), precision)
    if key not in _MODELS:
        d = GC.synth_weights(G.DualStyleGAN(size, 512, GC.N_MLP, GC.MULT), "generator.").to(device)
        for m in (d, d.generator):
            m.compute_dtype, m.exact_fp32 = PRECISIONS[precision]
        _MODELS[key] = {"d": d, "g": d.generator}
    return _MODELS[key]


def _move(v, device):
    if isinstance(v, torch.Tensor):
        return v.to(device)
    if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
        return [t.to(device) for t in v]
    return v


def _run_case(models, size, case, device):
    m, args, kw = GC.cases(size)[case]
    args = [_move(a, device) for a in args]
    kw = {k: _move(v, device) for k, v in kw.items()}
    return GC.outputs(models[m](*args, **kw))


def _golden(size, case):
    if case == "d4":
        return {"image": torch.from_numpy(GOLD[size]["g1.image"])}
    pre = case + "."
    return {k[len(pre):]: torch.from_numpy(v) for k, v in GOLD[size].items() if k.startswith(pre)}


def _check(got, want, precision, what):
    assert set(want) <= set(got), (what, sorted(got), sorted(want))
    rel_bar, psnr_bar = BARS[precision]
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        r = rel_err(g.numpy(), w.numpy())
        p = psnr(g.numpy(), w.numpy(), float(w.max() - w.min()))
        print(f"{what} {k}: max|d|/max|golden| {r:.3e} PSNR {p:.1f} dB")
        if k == "latent":
            assert r <= 1e-4, (what, k, r)          # the style path is fp32 in every precision
        else:
            assert r <= rel_bar and (psnr_bar is None or p >= psnr_bar), (what, k, r, p)


# ------------------------------------------------------------------------------------------------- 1. CPU dispatch
@pytest.mark.parametrize("case", CASES)
def test_cpu_dispatch_equals_reference(case):
    _lib.release_library()      # a CPU module of a user: no emulation bound
    models = _models(64, torch.device("cpu"))
    got, want = _run_case(models, 64, case, torch.device("cpu")), _golden(64, case)
    for k, w in want.items():
        r = rel_err(got[k].numpy(), w.numpy())
        assert got[k].shape == w.shape and r <= 1e-5, (case, k, r)
    assert isinstance(models["d"].executor(), G.EagerGenerator)


def test_cpu_dispatch_noise():
    _lib.release_library()
    g = _models(64, torch.device("cpu"))["g"]
    z = GC._rand(1, 2, 512)
    torch.manual_seed(3)
    a, _ = g([z])
    torch.manual_seed(3)
    maps = g.draw_noise(2)
    b, _ = g([z], noise=maps)
    torch.manual_seed(4)
    c, _ = g([z])
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert [m.shape for m in maps] == [(2, 1, h, w) for h, w in G.noise_sizes(64)]


# ------------------------------------------------------------------------------------------------- 2. the engine
def _size_for(dev):
    return 64 if dev.type == "cuda" else 32


def _bind(target):
    """What conftest's `dev` fixture does, for tests whose case list depends on the backend."""
    if target == "emu":
        from emu import build_emu
        _lib.use_library(build_emu.build())
        return torch.device("cpu")
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    _lib.use_library(_lib.DEFAULT_LIB)
    assert not _lib.is_emulation()
    return torch.device("cuda:0")


# host emulation (lanes as coroutines: ~20 s per case) runs the size-32 model: every case in fp32 and fp32_exact, and -- a cut of
# the case list that the MI355X run below does not make -- only the two cases with the most branches in bf16 and fp16, whose
# kernels differ from the fp32 ones in the element type alone; the MI355X: every case in every precision
ENGINE_RUNS = [("emu", c, p) for p in ("fp32", "fp32_exact") for c in CASES] + \
    [("emu", c, p) for c in ("g2", "d2") for p in ("bf16", "fp16")] + \
    [pytest.param("gpu", c, p, marks=pytest.mark.gpu) for p in PRECISIONS for c in CASES]


@pytest.mark.parametrize("target,case,precision", ENGINE_RUNS)
def test_engine_equals_reference(target, case, precision):
    dev = _bind(target)
    size = _size_for(dev)
    models = _models(size, dev, precision)
    assert isinstance(models["d"].executor(), G.GeneratorEngine)
    _check(_run_case(models, size, case, dev), _golden(size, case), precision, f"{case}/{precision}/{size}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["g1", "d1"])
def test_engine_full_size(case):
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    _lib.use_library(_lib.DEFAULT_LIB)
    dev = torch.device("cuda:0")
    models = _models(1024, dev)
    m, args, kw = GC.full_size_cases()[case]
    img, _ = models[m](*[_move(a, dev) for a in args], **kw)
    scale = max(float(np.abs(GOLD_FULL[f"{case}.{k}"]).max()) for k in ("pool", "centre", "corner"))
    for k, t in GC.reduce_full(img).items():
        w = GOLD_FULL[f"{case}.{k}"]
        r = float(np.abs(t.numpy() - w).max()) / scale
        print(f"{case}/1024 {k}: max|d|/max|golden| {r:.3e}")
        assert r <= 1e-4, (case, k, r)
    _MODELS.pop((1024, str(dev), "fp32"), None)   # ~1 GB of plans: not kept for the rest of the session


def test_engine_noise(dev):
    size = _size_for(dev)
    g = _models(size, dev)["g"]
    z = GC._rand(1, 2, 512).to(dev)
    torch.manual_seed(5)
    a, _ = g([z])
    torch.manual_seed(5)
    b, _ = g([z], randomize_noise=True)
    torch.manual_seed(5)
    maps = g.draw_noise(2)
    c, _ = g([z], noise=maps)
    torch.manual_seed(6)
    d, _ = g([z])
    assert torch.equal(a, b), "the same seed gives the same image"
    assert torch.equal(a, c), "draw_noise returns the maps of the randomised call"
    assert not torch.equal(a, d), "another seed gives another image"
    stored, _ = g([z], randomize_noise=False)
    assert not torch.equal(a, stored)
    # with every noise weight 0 the randomised call is the zero-noise call
    quiet = GC.synth_weights(G.Generator(size, 512, GC.N_MLP, GC.MULT), "generator.generator.")
    sd = quiet.state_dict()
    quiet.load_state_dict({k: torch.zeros_like(v) if k.endswith("noise.weight") else v for k, v in sd.items()})
    quiet = quiet.to(dev)
    torch.manual_seed(7)
    r, _ = quiet([z])
    zero, _ = quiet([z], noise=[torch.zeros_like(m) for m in maps])
    assert torch.equal(r, zero)


def test_weight_edit_rebuilds_the_engine(dev):
    size = _size_for(dev)
    g = GC.synth_weights(G.Generator(size, 512, GC.N_MLP, GC.MULT), "generator.generator.").to(dev)
    z = GC._rand(1, 1, 512).to(dev)
    a, _ = g([z], randomize_noise=False)
    e1 = g.executor()
    assert g.executor() is e1
    with torch.no_grad():
        g.to_rgb1.bias.add_(1.0)
    b, _ = g([z], randomize_noise=False)
    assert g.executor() is not e1 and not torch.equal(a, b)
    fresh = G.Generator(size, 512, GC.N_MLP, GC.MULT)
    fresh.load_state_dict({k: v.cpu() for k, v in g.state_dict().items()})
    c, _ = fresh.to(dev)([z], randomize_noise=False)
    assert torch.equal(b, c), "the edited module equals a module built from its weights"


# ------------------------------------------------------------------------------------------------- 3. surface
def test_signatures_and_schema():
    api = json.load(open(os.path.join(GOLDEN, "generator_api.json")))
    for name, cls in (("Generator", G.Generator), ("DualStyleGAN", G.DualStyleGAN)):
        for meth in ("__init__", "forward", "make_noise", "mean_latent", "get_latent"):
            sig = inspect.signature(getattr(cls, meth))
            got = [[p.name, None if p.default is inspect._empty else p.default] for p in sig.parameters.values()]
            got = [[n, list(d) if isinstance(d, (list, tuple)) else d] for n, d in got]
            assert got == api[name][meth], (name, meth, got)
    d = G.DualStyleGAN(1024, 512, 8, 2)
    keys_d = load_keys("D")
    want = {k[len("generator."):]: v for k, v in keys_d.items() if k.startswith("generator.")}
    assert {k: tuple(v.shape) for k, v in d.state_dict().items()} == want
    want_g = {k[len("generator.generator."):]: v for k, v in keys_d.items() if k.startswith("generator.generator.")}
    assert {k: tuple(v.shape) for k, v in d.generator.state_dict().items()} == want_g
    assert isinstance(d.generator, G.Generator) and d.res_index == 6 and d.n_latent == 18
    assert [tuple(n.shape) for n in d.make_noise()] == [(1, 1, h, w) for h, w in G.noise_sizes(1024)]


def test_vtoonify_generator_runs_and_forward_is_unchanged(dev):
    """VToonify(...).generator(...) and .stylegan()(...) work after load_state_dict, in the module's precision, and
    VToonify.forward on the golden case of tests/golden/e2e_D.npz gives the reference's frame and the same bits before and after
    the generator calls.  Host emulation stops the 1024^2 generators at their early returns (8^2 and 32^2: what a coroutine
    run can afford); the MI355X also runs both to the image and holds DualStyleGAN's against the full-size golden."""
    d, _ = load_golden("e2e_D.npz")
    model = VToonify(in_size=256, out_size=1024, backbone="dualstylegan")
    assert len(model.state_dict()) == 399
    assert isinstance(model.generator, G.DualStyleGAN) and isinstance(model.stylegan(), G.Generator)
    assert model.generator.compute_dtype == model.stylegan().compute_dtype == model.compute_dtype
    model.load_state_dict(synth.synth_state_dict(load_keys("D")))
    model = model.to(dev)
    x, style = torch.from_numpy(d["x"]).to(dev), torch.from_numpy(d["style"]).to(dev)
    before = model(x, style, d_s=0.5).clone()
    assert rel_err(before.cpu().numpy(), d["y_ds0.5"]) <= 1e-4
    z, ex = GC._rand(1, 1, 512).to(dev), GC._rand(3, 1, 512).to(dev)
    feat, skip = model.stylegan()([z], randomize_noise=False, return_feature_ind=1)
    assert feat.shape == (1, 512, 8, 8) and skip.shape == (1, 3, 8, 8) and torch.isfinite(feat).all()
    feat, skip = model.generator([z], ex, randomize_noise=False, return_feat=True)
    assert feat.shape == (1, 512, 32, 32) and skip.shape == (1, 3, 32, 32) and torch.isfinite(feat).all()
    if dev.type == "cuda":
        img, _ = model.generator([z], ex, randomize_noise=False)
        img_g, _ = model.stylegan()([z], randomize_noise=False)
        assert img.shape == img_g.shape == (1, 3, 1024, 1024) and torch.isfinite(img_g).all()
        scale = max(float(np.abs(GOLD_FULL[f"d1.{k}"]).max()) for k in ("pool", "centre", "corner"))
        for k, t in GC.reduce_full(img).items():
            assert float(np.abs(t.numpy() - GOLD_FULL[f"d1.{k}"]).max()) <= 1e-4 * scale, k
    after = model(x, style, d_s=0.5)
    assert torch.equal(before, after)
