"""What the MS-SSIM perceptual term adds to a C5 training step (bench.py --config c5: HVAE encoder(1024) on 256^2
through a frozen SG3-T-256, batch 16, f16 with the loss scaler): the same step with perceptual_weight=0 and with
perceptual_weight=0.8, percep=metrics.MSSSIMLoss(), timed in alternating blocks.  Prints one JSON line.

    python tools/bench_c5_percep.py [--batch 16] [--steps 10] [--warmup 3] [--precision f16|bf16|fp32]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_compression_2_amd as ic2  # noqa: E402
from image_compression_2_amd import training as ict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="f16")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    prec = args.precision
    torch.manual_seed(0)
    enc = ic2.HVAE_VGG_Encoder(img_resolution=1024, precision=prec).to(dev)
    torch.manual_seed(1)
    G = ic2.Generator(img_resolution=256, precision=prec).to(dev).eval()
    comp = ic2.StyleGAN3Compressor(enc, G, training_resolution=256)
    x = (torch.rand(args.batch, 3, 256, 256, generator=torch.Generator().manual_seed(1000)) * 2 - 1).to(dev)
    opt = ict.make_optimizer(enc, lr=1e-4)
    w_avg = G.mapping.w_avg.view(1, 1, -1)
    scaler = ict.make_f16(comp) if prec == "f16" else None
    percep = ic2.MSSSIMLoss()

    def step(weight):
        return ict.train_step(comp, x, opt, w_avg, rec_weight=1.0, perceptual_weight=weight, kl_weight=0.01,
                              percep=percep if weight else None, scaler=scaler)

    def timed(weight):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = step(weight)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out
    times = {0.0: [], 0.8: []}
    last = {}
    for it in range(args.warmup + args.steps):
        for weight in (0.0, 0.8):
            ms, out = timed(weight)
            last[weight] = out
            if it >= args.warmup:
                times[weight].append(ms)
    base, with_term = statistics.median(times[0.0]), statistics.median(times[0.8])
    print(json.dumps({"config": "c5", "batch": args.batch, "precision": prec, "steps": args.steps,
                      "step_ms": {"perceptual_weight_0": round(base, 3), "ms_ssim_0.8": round(with_term, 3)},
                      "added_ms": round(with_term - base, 3), "added_pct": round(100 * (with_term / base - 1), 2),
                      "img_per_s": {"perceptual_weight_0": round(args.batch / base * 1e3, 1),
                                    "ms_ssim_0.8": round(args.batch / with_term * 1e3, 1)},
                      "perceptual_loss": float(last[0.8]["perceptual_loss"]),
                      "rec_loss": float(last[0.8]["rec_loss"])}))


if __name__ == "__main__":
    main()
