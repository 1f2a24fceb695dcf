"""MS-SSIM on the HIP path against the same definition composed from torch ops on the GPU (F.conv2d with the
separable 11-tap window, F.avg_pool2d, autograd), which is what a user would run without it.  At batch 16 and 32,
3 x 256^2 and 3 x 1024^2: medians of interleaved calls for the forward (loss mode) and for forward + backward (the
gradient with respect to the reconstruction, as train_step takes it), and both sides' ratio to their algorithmic HBM
bytes at 8 TB/s: forward = one read of both images (8 B / pixel), forward + backward = two reads of both and one
write of the gradient (20 B / pixel).  Prints one JSON line per configuration.

    python tools/bench_ms_ssim.py [--steps 10] [--warmup 2] [--shapes 16x256,32x256,16x1024,32x1024]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_compression_2_amd import metrics as icm  # noqa: E402

HBM_BYTES_PER_S = 8e12


def torch_loss(a, b, g):
    """1 - MS-SSIM per image of x*0.5+0.5 with data range 1, composed from torch ops (f32)."""
    n, c, h, w = a.shape
    x = (a * 0.5 + 0.5).reshape(n * c, 1, h, w)
    y = (b * 0.5 + 0.5).reshape(n * c, 1, h, w)
    gh, gv = g.view(1, 1, 1, 11), g.view(1, 1, 11, 1)
    filt = lambda t: F.conv2d(F.conv2d(t, gh), gv)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    terms = []
    for s in range(5):
        mx, my = filt(x), filt(y)
        sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
        m = (2 * sxy + c2) / (sxx + syy + c2)
        if s == 4:
            m = m * (2 * mx * my + c1) / (mx * mx + my * my + c1)
        terms.append(m.mean(dim=(1, 2, 3)))
        if s < 4:
            ph, pw = x.shape[2] % 2, x.shape[3] % 2
            x, y = F.avg_pool2d(x, 2, padding=(ph, pw)), F.avg_pool2d(y, 2, padding=(ph, pw))
    t = torch.stack(terms, dim=1).reshape(n, c, 5)
    wts = torch.tensor(icm.MS_SSIM_WEIGHTS, device=a.device)
    return 1.0 - (t.clamp_min(0) ** wts).prod(dim=2).mean(dim=1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="16x256,32x256,16x1024,32x1024")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    i = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2))
    g = (g / g.sum()).float().to(dev)
    for spec in args.shapes.split(","):
        n, side = (int(v) for v in spec.split("x"))
        gen = torch.Generator(device=dev).manual_seed(n + side)
        a = torch.rand(n, 3, side, side, generator=gen, device=dev) * 2 - 1
        b = (a + 0.05 * torch.randn(a.shape, generator=gen, device=dev)).requires_grad_(True)

        def hip_fwd():
            with torch.no_grad():
                return icm.ms_ssim_loss(a, b)

        def hip_fwd_bwd():
            return torch.autograd.grad(icm.ms_ssim_loss(a, b).mean(), b)[0]

        def torch_fwd():
            with torch.no_grad():
                return torch_loss(a, b, g)

        def torch_fwd_bwd():
            return torch.autograd.grad(torch_loss(a, b, g).mean(), b)[0]
        fns = {"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_fwd_bwd": hip_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd}
        times = {k: [] for k in fns}
        for it in range(args.warmup + args.steps):
            for k, fn in fns.items():          # interleaved: every iteration times each variant once
                ms = timed(fn)
                if it >= args.warmup:
                    times[k].append(ms)
        med = {k: statistics.median(v) for k, v in times.items()}
        pixels = n * 3 * side * side
        floor = {"fwd": 8 * pixels / HBM_BYTES_PER_S * 1e3, "fwd_bwd": 20 * pixels / HBM_BYTES_PER_S * 1e3}
        value_diff = (hip_fwd() - torch_fwd()).abs().max().item()
        grad_diff = (hip_fwd_bwd() - torch_fwd_bwd()).abs().max().item()
        print(json.dumps({
            "batch": n, "side": side, "steps": args.steps,
            "ms": {k: round(v, 4) for k, v in med.items()},
            "hbm_floor_ms": {k: round(v, 4) for k, v in floor.items()},
            "x_floor": {"hip_fwd": round(med["hip_fwd"] / floor["fwd"], 1),
                        "torch_fwd": round(med["torch_fwd"] / floor["fwd"], 1),
                        "hip_fwd_bwd": round(med["hip_fwd_bwd"] / floor["fwd_bwd"], 1),
                        "torch_fwd_bwd": round(med["torch_fwd_bwd"] / floor["fwd_bwd"], 1)},
            "speedup_vs_torch": {"fwd": round(med["torch_fwd"] / med["hip_fwd"], 2),
                                 "fwd_bwd": round(med["torch_fwd_bwd"] / med["hip_fwd_bwd"], 2)},
            "max_abs_diff_vs_torch": {"loss": value_diff, "grad": grad_diff}}), flush=True)


if __name__ == "__main__":
    main()
