"""Cost of the fused PSNR + SSIM pass (ic2_uint8_quality) against the PSNR-only pass (ic2_uint8_sse) at the C2 metric
shape (32, 3, 256, 256) and the C4 shape (8, 3, 1024, 1024): device-event time of each (median over batches of
back-to-back launches on preallocated outputs, after warm-up), their ratio, and the fused pass's HBM floor: two reads
of N*C*H*W*4 bytes at the device-to-device copy bandwidth measured in the same run on a buffer of the same size.

    python tools/bench_quality.py [--reps 30] [--inner 20] [--win 7]

One GPU process; a machine without a ROCm device fails (no fallback).  The inputs at these shapes (25 / 101 MB each)
fit the 256 MiB Infinity Cache, and so does the copy the floor is taken from: the floor is the same-footprint copy
rate, not the HBM peak.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("C2 metric", (32, 3, 256, 256)), ("C4", (8, 3, 1024, 1024))]


def timed(fn, reps, inner, warmup=3):
    """Median milliseconds per call of `fn` over `reps` batches of `inner` back-to-back launches."""
    for _ in range(warmup * inner):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--win", type=int, default=7)
    args = ap.parse_args()
    from image_compression_2_amd import _native as nv
    dev = torch.device("cuda", 0)
    print(f"device {torch.cuda.get_device_name(0)}; win {args.win}; median (min .. max) of {args.reps} batches of "
          f"{args.inner} launches")
    for label, shape in SHAPES:
        n, c, h, w = shape
        g = torch.Generator(device=dev).manual_seed(1)
        a = torch.rand(shape, device=dev, generator=g) * 2.4 - 1.2
        b = torch.rand(shape, device=dev, generator=g) * 2 - 1
        nbytes = a.numel() * 4
        st = nv.stream_of(a)
        sse = torch.empty(n, dtype=torch.float64, device=dev)
        sse_q = torch.empty(n, dtype=torch.float64, device=dev)
        ssim_sum = torch.empty(n, c, dtype=torch.float64, device=dev)
        s_sse = torch.empty(int(nv.query("ic2_uint8_sse_scratch_doubles", n)), dtype=torch.float64, device=dev)
        s_q = torch.empty(int(nv.query("ic2_uint8_quality_scratch_doubles", n, c, h, w, args.win)),
                          dtype=torch.float64, device=dev)
        dst = torch.empty_like(a)

        def run_sse():
            nv.call("ic2_uint8_sse", nv.ptr(a), nv.ptr(b), n, c * h * w, nv.ptr(sse), nv.ptr(s_sse), st)

        def run_quality():
            nv.call("ic2_uint8_quality", nv.ptr(a), nv.ptr(b), n, c, h, w, args.win, nv.ptr(sse_q), nv.ptr(ssim_sum),
                    nv.ptr(s_q), st)

        t_copy = timed(lambda: dst.copy_(a), args.reps, args.inner)
        t_sse = timed(run_sse, args.reps, args.inner)
        t_q = timed(run_quality, args.reps, args.inner)
        assert torch.equal(sse, sse_q), "the two passes disagree on the squared error"
        copy_bw = 2 * nbytes / (t_copy[0] * 1e-3)          # a copy reads and writes its bytes
        floor_ms = 2 * nbytes / copy_bw * 1e3              # the fused pass reads both images once
        print(f"[{label}] shape {shape}: {nbytes / 1e6:.1f} MB per image batch")
        print(f"  copy (d2d, same size)   {t_copy[0] * 1e3:9.1f} us ({t_copy[1] * 1e3:.1f} .. {t_copy[2] * 1e3:.1f})"
              f"  -> {copy_bw / 1e12:.2f} TB/s read + write")
        print(f"  ic2_uint8_sse           {t_sse[0] * 1e3:9.1f} us ({t_sse[1] * 1e3:.1f} .. {t_sse[2] * 1e3:.1f})"
              f"  -> {2 * nbytes / (t_sse[0] * 1e-3) / 1e12:.2f} TB/s read")
        print(f"  ic2_uint8_quality       {t_q[0] * 1e3:9.1f} us ({t_q[1] * 1e3:.1f} .. {t_q[2] * 1e3:.1f})"
              f"  -> {2 * nbytes / (t_q[0] * 1e-3) / 1e12:.2f} TB/s read")
        print(f"  quality / sse           {t_q[0] / t_sse[0]:9.2f} x")
        print(f"  floor (2 reads at the copy rate) {floor_ms * 1e3:.1f} us; quality / floor {t_q[0] / floor_ms:.2f} x")


if __name__ == "__main__":
    main()
