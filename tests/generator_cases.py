"""The cases of tests/golden/generator*.npz, shared by tests/golden/make_golden_generator.py (which runs them on the reference's
Generator / DualStyleGAN) and tests/test_generator.py (which runs them on vtoonify_amd.generator).  Inputs are not stored: both
sides draw them here from seeded CPU generators; weights come from vtoonify_amd.synth under the key names the tensors have
in a VToonify state_dict.

Every case: (model, keyword arguments of forward) -> (first output, second output).  Large feature outputs are compared on
every `FEAT_STRIDE`-th channel (a (2,512,32,32) tensor would not fit the size limit of a committed file).
"""
import torch

from vtoonify_amd import synth

N_MLP, MULT, B = 8, 2, 2
FEAT_STRIDE = 32


def synth_weights(module, prefix):
    """Load synthetic weights into a Generator (prefix 'generator.generator.') or DualStyleGAN ('generator.'): the values a
    VToonify-D state_dict built by synth would hold under those names."""
    sd = {k: synth.synth_tensor(prefix + k, v.shape).to(v.dtype) for k, v in module.state_dict().items()}
    module.load_state_dict(sd)
    return module


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def noise_list(size, seed, batch):
    log_size = size.bit_length() - 1
    return [_rand(seed + i, batch, 1, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2)) for i in range(2 * (log_size - 2) + 1)]


def cases(size):
    """{name: (model, args, kwargs)}; model 'g' = Generator, 'd' = DualStyleGAN."""
    n_latent = 2 * (size.bit_length() - 1) - 2
    z1, z2, ex = _rand(1, B, 512), _rand(2, B, 512), _rand(3, B, 512)
    wplus, explus, zplus = _rand(4, B, n_latent, 512) * 0.5, _rand(5, B, n_latent, 512), _rand(6, B, n_latent, 512)
    mean_w = _rand(7, 1, 512) * 0.3
    iw = [0.75, 0.0, 0.5, 1.0, 0.25, 0.6, 0.9, 0.3, 0.8, 0.45, 0.2, 0.7, 0.35, 0.65, 0.15, 0.85, 0.55, 0.95][:n_latent]
    iw = iw + [1.0] * (18 - len(iw))
    return {
        "g1": ("g", [[z1]], dict(randomize_noise=False, return_latents=True)),
        "g2": ("g", [[z1, z2]], dict(inject_index=3, truncation=0.7, truncation_latent=mean_w, noise=noise_list(size, 100, B))),
        "g3": ("g", [[wplus]], dict(input_is_latent=True, return_feature_ind=3, randomize_noise=False)),
        "g4": ("g", [[zplus]], dict(z_plus_latent=True, randomize_noise=False)),
        "d1": ("d", [[z1], ex], dict(randomize_noise=False)),
        "d2": ("d", [[wplus], explus], dict(input_is_latent=True, interp_weights=iw, randomize_noise=False)),
        "d3": ("d", [[z1], ex], dict(fuse_index=4, randomize_noise=False)),
        "d4": ("d", [[z1], ex], dict(use_res=False, randomize_noise=False)),          # equals g1's image
        "d5": ("d", [[z1], ex], dict(return_feat=True, randomize_noise=False)),
    }


def full_size_cases():
    z1, ex = _rand(1, 1, 512), _rand(3, 1, 512)
    return {"g1": ("g", [[z1]], dict(randomize_noise=False)), "d1": ("d", [[z1], ex], dict(randomize_noise=False))}


def reduce_full(img):
    """(1,3,1024,1024) -> the three views the golden stores: 8x8 average pool, centre crop, corner crop."""
    img = img.detach().float().cpu()
    return {"pool": torch.nn.functional.avg_pool2d(img, 8)[0], "centre": img[0, :, 480:544, 480:544], "corner": img[0, :, :64, :64]}


def outputs(result):
    """forward's pair -> {suffix: tensor} as stored."""
    a, b = result
    out = {}
    if a.ndim == 4 and a.shape[1] > 3:            # (feature, skip)
        out["feat"], out["skip"] = a[:, ::FEAT_STRIDE], b
    else:
        out["image"] = a
        if b is not None:
            out["latent"] = b
    return {k: v.detach().float().cpu().contiguous() for k, v in out.items()}
