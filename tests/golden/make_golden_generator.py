#!/usr/bin/env python3
"""Generate tests/golden/generator.npz (size 64), generator_32.npz (the emulated suite's model) and generator_1024.npz (one
full-size case, reduced) from the REAL reference's Generator and DualStyleGAN.

Runs only where the reference tree is available (VTOONIFY_REFERENCE, read-only).  As make_golden.py does, the reference's CPU
operator twin is selected by aliasing sys.modules['model.stylegan.op'] -> model.stylegan.op_cpu before the model is imported.
Nothing is copied from the reference: only tensors it computes.  Weights and inputs are not stored: tests/generator_cases.py
rebuilds both from seeds on either side.  Three files because one would exceed the size limit of a committed file.

    python tests/golden/make_golden_generator.py [--no-1024 | --api-only]
"""
import importlib
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VTOONIFY_REFERENCE", "/root/reference")

sys.path.insert(0, REF)
import model.stylegan  # noqa: E402  (the reference's package)

_cpu = importlib.import_module("model.stylegan.op_cpu")
_gf = importlib.import_module("model.stylegan.op_cpu.conv2d_gradfix")
sys.modules["model.stylegan.op"] = _cpu
sys.modules["model.stylegan.op.conv2d_gradfix"] = _gf
_cpu.conv2d_gradfix = _gf

import numpy as np  # noqa: E402
import torch  # noqa: E402
from model.dualstylegan import DualStyleGAN  # noqa: E402
from model.stylegan.model import Generator  # noqa: E402

sys.path.append(REPO)
sys.path.append(os.path.join(REPO, "tests"))
import generator_cases as GC  # noqa: E402

torch.set_grad_enabled(False)


def build(size):
    d = GC.synth_weights(DualStyleGAN(size, 512, GC.N_MLP, GC.MULT).eval(), "generator.")
    return {"d": d, "g": d.generator}


def save(name, arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **{k: np.ascontiguousarray(v.numpy()) for k, v in arrays.items()})
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")
    assert os.path.getsize(path) < (1 << 20)


def save_api():
    """Names and defaults of the public methods (tests/golden/generator_api.json): no code, only what a caller types."""
    import inspect
    import json
    api = {}
    for name, cls in (("Generator", Generator), ("DualStyleGAN", DualStyleGAN)):
        api[name] = {}
        for meth in ("__init__", "forward", "make_noise", "mean_latent", "get_latent"):
            ps = inspect.signature(getattr(cls, meth)).parameters.values()
            api[name][meth] = [[p.name, None if p.default is inspect._empty else p.default] for p in ps]
    with open(os.path.join(HERE, "generator_api.json"), "w") as f:
        json.dump(api, f, indent=1)
        f.write("\n")
    print("wrote generator_api.json")


def main():
    save_api()
    if "--api-only" in sys.argv:
        return
    for size, name in ((64, "generator.npz"), (32, "generator_32.npz")):
        models, out = build(size), {}
        for case, (m, args, kw) in GC.cases(size).items():
            if case == "d4":
                img, _ = models[m](*args, **kw)
                ref, _ = models["g"](*GC.cases(size)["g1"][1], randomize_noise=False)
                assert torch.equal(img, ref), "use_res=False is the plain generator"
                continue
            for suffix, t in GC.outputs(models[m](*args, **kw)).items():
                out[f"{case}.{suffix}"] = t
        save(name, out)
    if "--no-1024" not in sys.argv:
        models, out = build(1024), {}
        for case, (m, args, kw) in GC.full_size_cases().items():
            img, _ = models[m](*args, **kw)
            for suffix, t in GC.reduce_full(img).items():
                out[f"{case}.{suffix}"] = t.contiguous()
        save("generator_1024.npz", out)


if __name__ == "__main__":
    main()
