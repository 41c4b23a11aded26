#!/usr/bin/env python3
"""DualStyleGAN portrait stylisation of a face, or samples of the StyleGAN2 generator, on vtoonify_amd.generator.

    python tools/generate_amd.py --ckpt vtoonify_s_d.pt --style_encoder_path encoder.pt --content face.jpg \\
        --exstyle_path exstyle_code.npy --style_id 26 --weight 0.75 0.75 ... (18 floats)          # portrait at 1024^2
    python tools/generate_amd.py --ckpt vtoonify_s_d.pt --content photo.npy --landmarks lm.npy ...  # aligned here, no dlib
    python tools/generate_amd.py --ckpt synthetic --size 64 --seed 3                               # samples Generator

With --content the chain is the one of tools/style_transfer_amd.py (its `style_input`): face -> alignment (the reference's
align_face when dlib is importable, vtoonify_amd/align.py from --landmarks (68,2) otherwise, else the image as given, resized to
256^2) -> pSp z+ code (+ latent_avg) -> `zplus2wplus` (the generator's mapping network) -> W+; the extrinsic code of --style_id
from --exstyle_path goes through the same mapping, as it does there; then
`DualStyleGAN([w+], exstyle, input_is_latent=True, interp_weights=--weight)`.  --content is an image file (cv2, BGR on disk) or
an (H,W,3) uint8 RGB .npy.  --intrinsic_code replaces the encoder with a stored z+ code (18,512) -- the meaning the option has
in tools/style_transfer_amd.py.  A model smaller than 1024^2 (`--size`, synthetic weights) reads the first n_latent rows.
Without --content and --intrinsic_code the tool samples `Generator([z])` with one z drawn from --seed.

`--ckpt synthetic` / `--style_encoder_path synthetic` build seeded random weights (vtoonify_amd.synth); with synthetic weights
and no file at --exstyle_path the extrinsic code is synthetic too.  A checkpoint holds the reference's `g_ema` state_dict of a
VToonify-D (keys `generator.*`) or of a DualStyleGAN.  Output: <output_path>/generate.npy, (1,3,H,W) fp32 un-clamped, plus
generate.png when cv2 is importable.  Noise is drawn by the package's own counter-based generator from --seed (not torch's
`normal_` bits): the same seed gives the same bytes.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vtoonify_amd import generator as G, synth  # noqa: E402

PRECISIONS = {"fp32": (torch.float32, False), "fp32_exact": (torch.float32, True), "bf16": (torch.bfloat16, False),
              "fp16": (torch.float16, False)}


def parse(argv=None):
    p = argparse.ArgumentParser(description="Generator / DualStyleGAN forward on the MI355X")
    p.add_argument("--ckpt", type=str, default="./checkpoint/vtoonify_d_cartoon/vtoonify_s_d.pt", help="path of the saved model, or `synthetic`")
    p.add_argument("--style_encoder_path", type=str, default="./checkpoint/encoder.pt", help="path of the style encoder, or `synthetic`")
    p.add_argument("--exstyle_path", type=str, default=None, help="path of the extrinsic style codes (default: beside --ckpt)")
    p.add_argument("--style_id", type=int, default=26, help="the id of the style image")
    p.add_argument("--content", type=str, default=None, help="the face: an image file or an (H,W,3) uint8 RGB .npy")
    p.add_argument("--landmarks", type=str, default=None, help=".npy (68,2) landmarks of --content: align it here, without dlib")
    p.add_argument("--intrinsic_code", type=str, default=None, help=".npy z+ code (18,512) instead of the style encoder")
    p.add_argument("--weight", type=float, nargs=18, default=[0.75] * 7 + [1.0] * 11, help="interp_weights: structure, then colour")
    p.add_argument("--truncation", type=float, default=1.0, help="truncation psi towards the mean latent of 4096 samples")
    p.add_argument("--seed", type=int, default=0, help="seed of the noise, of the sampled z and of `synthetic` weights")
    p.add_argument("--precision", choices=list(PRECISIONS), default="fp32")
    p.add_argument("--output_path", type=str, default="./output/")
    p.add_argument("--size", type=int, default=1024, help="output size of the model")
    opt = p.parse_args(argv)
    if opt.exstyle_path is None:
        opt.exstyle_path = os.path.join(os.path.dirname(opt.ckpt), "exstyle_code.npy")
    return opt


def load_model(opt, device):
    model = G.DualStyleGAN(opt.size, 512, 8, 2)
    if opt.ckpt.startswith("synthetic"):
        sd = {k: synth.synth_tensor("generator." + k, v.shape, opt.seed).to(v.dtype) for k, v in model.state_dict().items()}
    else:
        ck = torch.load(opt.ckpt, map_location="cpu")
        sd = ck.get("g_ema", ck)
        if any(k.startswith("generator.generator.") for k in sd):      # a VToonify-D checkpoint
            sd = {k[len("generator."):]: v for k, v in sd.items() if k.startswith("generator.")}
    model.load_state_dict(sd)
    model = model.to(device)
    for m in (model, model.generator):
        m.compute_dtype, m.exact_fp32 = PRECISIONS[opt.precision]
    return model


def read_face(path):
    """(H,W,3) uint8 RGB."""
    if path.endswith(".npy"):
        face = np.load(path)
    else:
        try:
            import cv2
        except ImportError:
            raise SystemExit(f"--content {path}: reading an image file needs cv2; pass an (H,W,3) uint8 RGB .npy") from None
        face = cv2.imread(path)
        if face is None:
            raise SystemExit(f"--content {path}: not readable")
        face = face[..., ::-1]
    if face.ndim != 3 or face.shape[2] != 3 or face.dtype != np.uint8:
        raise SystemExit("--content: expected an (H,W,3) uint8 image")
    return np.ascontiguousarray(face)


def zplus_code(opt, device, log=print):
    """pSp's z+ code (1,18,512) of --content (style_transfer.py:135-147), or the stored --intrinsic_code."""
    if opt.intrinsic_code:
        return torch.from_numpy(np.load(opt.intrinsic_code)).float().reshape(1, 18, 512).to(device)
    from style_transfer_amd import _shapes, style_input
    from vtoonify_amd import psp
    lm = np.load(opt.landmarks) if opt.landmarks else None
    t = style_input(opt, read_face(opt.content), False, device, log, lm)
    dt = PRECISIONS[opt.precision][0]
    enc = psp.GradualStyleEncoder(50, "ir_se", compute_dtype=torch.float32 if device.type == "cpu" else dt)
    if opt.style_encoder_path.startswith("synthetic"):
        enc.load_state_dict(synth.synth_state_dict(_shapes("psp"), opt.seed))
        latent_avg = torch.zeros(18, 512)
    else:
        ck = torch.load(opt.style_encoder_path, map_location="cpu")               # util.py:150-160
        enc.load_state_dict({k[len("encoder."):]: v for k, v in ck["state_dict"].items() if k.startswith("encoder.")})
        latent_avg = ck["latent_avg"]
    enc.eval().to(device)
    with torch.no_grad():
        return enc(t).float() + latent_avg.to(device).reshape(1, -1, 512)


def exstyle_code(opt, device):
    """The z+ code (1,18,512) of --style_id: the reference's exstyle_code.npy is a dict name -> code, taken in key order
    (style_transfer.py:83)."""
    if opt.ckpt.startswith("synthetic") and not os.path.exists(opt.exstyle_path):
        return synth.synth_style(seed=100 + opt.style_id).to(device)
    exstyles = np.load(opt.exstyle_path, allow_pickle=True).item()
    return torch.tensor(exstyles[list(exstyles.keys())[opt.style_id]]).float().reshape(1, 18, 512).to(device)


def zplus2wplus(model, z):
    """The generator's mapping network on every row (model/vtoonify.py:285-286), rows cut to the model's n_latent."""
    z = z[:, :model.n_latent].contiguous()
    return model.get_latent(z.reshape(-1, z.shape[-1])).reshape(z.shape)


def main(argv=None, device=None):
    opt = parse(argv)
    device = torch.device(device if device is not None else "cuda:0")
    model = load_model(opt, device)
    portrait = bool(opt.content or opt.intrinsic_code)
    if portrait:
        w = zplus2wplus(model, zplus_code(opt, device))
        ex = zplus2wplus(model, exstyle_code(opt, device))
    # seeded here, after every module is built (constructors draw their initial weights from the same generator): what
    # follows -- the mean latent, the sampled z, the key of the noise -- is a function of --seed alone
    torch.manual_seed(opt.seed)
    kw = {}
    if opt.truncation < 1:
        kw["truncation"], kw["truncation_latent"] = opt.truncation, model.mean_latent(4096)
    if portrait:
        img, _ = model([w], ex, input_is_latent=True, interp_weights=list(opt.weight), **kw)
    else:
        img, _ = model.generator([torch.randn(1, 512).to(device)], **kw)
    img = img.float().cpu().numpy()
    os.makedirs(opt.output_path, exist_ok=True)
    path = os.path.join(opt.output_path, "generate.npy")
    np.save(path, img)
    try:
        import cv2
        u8 = ((np.clip(img[0].transpose(1, 2, 0), -1, 1) + 1.0) * 127.5).astype(np.uint8)        # tensor2cv2, util.py:190-192
        cv2.imwrite(os.path.join(opt.output_path, "generate.png"), np.ascontiguousarray(u8[:, :, ::-1]))
    except ImportError:
        pass
    print(f"generate_amd: {path} {img.shape} precision {opt.precision if device.type != 'cpu' else 'fp32 (torch, CPU)'}")
    return {"path": path, "image": img}


if __name__ == "__main__":
    main()
