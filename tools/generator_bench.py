#!/usr/bin/env python3
"""Time Generator.forward and DualStyleGAN.forward at 1024^2 on one MI355X.

    python tools/generator_bench.py [--size 1024] [--iters 10] > profiles/generator_bench.txt

B in {1, 4}, bf16 and fp32 (three-term bf16 products), with zero noise (a list of zero maps), the stored `noises.noise_i`
buffers and randomised noise.  Per row: milliseconds per forward call (HIP events around `iters` calls after 3 warm-up
calls, host dispatch included: the calls are not graph-captured), and the share of that time which the plan's
vt_noise_bias_act launches and -- randomised noise only -- the vt_randn launches take when they are replayed alone.
Synthetic weights; there is no throughput bar for this path.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vtoonify_amd import generator as G, synth  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=1024)
    p.add_argument("--iters", type=int, default=10)
    opt = p.parse_args()
    dev = torch.device("cuda:0")
    base = G.DualStyleGAN(opt.size, 512, 8, 2)
    base.load_state_dict({k: synth.synth_tensor("generator." + k, v.shape).to(v.dtype) for k, v in base.state_dict().items()})
    print(f"# generator_bench: size {opt.size}, {torch.cuda.get_device_name(0)}, {opt.iters} calls per figure")
    print("model         B  dtype  noise       ms/call   noise_bias_act ms (share)   randn ms (share)")
    for dtype, dname in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        model = base.to(dev)
        for m in (model, model.generator):
            m.compute_dtype, m.exact_fp32 = dtype, False
        for B in (1, 4):
            g = torch.Generator().manual_seed(B)
            z, ex = torch.randn(B, 512, generator=g).to(dev), torch.randn(B, 512, generator=g).to(dev)
            zeros = [torch.zeros(1, 1, h, w, device=dev) for h, w in G.noise_sizes(opt.size)]
            for name, call in (("Generator", lambda **kw: model.generator([z], **kw)),
                               ("DualStyleGAN", lambda **kw: model([z], ex, **kw))):
                for mode, kw in (("zero", dict(noise=zeros)), ("stored", dict(randomize_noise=False)),
                                 ("randomised", dict(randomize_noise=True))):
                    ms = timed(lambda: call(**kw), opt.iters)
                    eng = (model.generator if name == "Generator" else model).executor()
                    plan = eng.last_plan      # the plan of the calls just timed
                    nba = [op for op in plan.ops if isinstance(op[2], dict) and op[2]["name"] == "noise_bias_act"]
                    t_nba = timed(lambda: eng.run_ops(nba), opt.iters)
                    t_rn = 0.0
                    if mode == "randomised":
                        t_rn = timed(lambda: [G.randn_into(nz, 12345, j) for j, nz in enumerate(plan.noise)], opt.iters)
                    print(f"{name:<13s} {B}  {dname:<5s}  {mode:<10s}  {ms:8.3f}   {t_nba:7.3f} ({100 * t_nba / ms:4.1f} %)"
                          f"          {t_rn:7.3f} ({100 * t_rn / ms:4.1f} %)", flush=True)
        del model
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
