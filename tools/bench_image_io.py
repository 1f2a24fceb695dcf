"""Cost of the device-side image I/O (image_io.py: ic2_resample_u8, ic2_image_to_u8) and of the CPU pipeline it
replaces, in one run:

  1. N = 32 RGB images 1024 x 1024 -> 256 x 256, LANCZOS, to the normalised f32 NCHW batch (to_tensor);
  2. N = 32 RGB images of seeded sizes 300 .. 600 per side -> 256 x 256, one ragged call;
  3. to_uint8 of a 32 x 3 x 256 x 256 batch, each mode.

For each: device-event time per call (median over batches of back-to-back calls on warmed caches; a resample call is
two launches), the bytes the algorithm must move computed from the shapes (sources rows read once + output written;
the workspace's write and read are listed apart) over that time against the HBM peak, the host-to-device time of the
uint8 sources from pinned memory, and PIL's resize + the same table on a 16-thread pool over the same images.

    python tools/bench_image_io.py [--reps 20] [--inner 10] [--threads 16]

One GPU process; a machine without a ROCm device fails (no fallback).  The sources (100 MB and about 19 MB) fit the
256 MiB Infinity Cache, so repeated calls read them from there: the shares of the HBM peak are upper bounds of what a
cold call reaches.
"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12       # bytes / s, specification
HBM_MEASURED = 6.29e12  # bytes / s, a float4 copy


def timed(fn, reps, inner, warmup=2):
    """Median (min, max) milliseconds per call of `fn` over `reps` batches of `inner` back-to-back calls."""
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


def fmt(t):
    return f"{t[0] * 1e3:9.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f})"


def resample_workload(label, images, res, args, dev):
    from image_compression_2_amd import image_io, ops
    n, c = len(images), 3
    sizes = [(i.shape[0], i.shape[1]) for i in images]
    src_bytes = sum(h * w * c for h, w in sizes)
    blob = torch.empty(src_bytes, dtype=torch.uint8).pin_memory()
    off = 0
    for i in images:
        blob[off:off + i.size] = torch.from_numpy(i).reshape(-1)
        off += i.size
    on_dev = torch.empty(src_bytes, dtype=torch.uint8, device=dev)
    t_h2d = timed(lambda: on_dev.copy_(blob, non_blocking=True), args.reps, args.inner)
    # the two launches alone, on sources already resident and preallocated workspace and outputs
    code = image_io._filter_code("lanczos")
    arena, (recs, max_rows, total_rows) = image_io._plan(sizes, res, res, c, code, dev)
    ws = torch.empty(total_rows * res * c, dtype=torch.uint8, device=dev)
    out = torch.empty(n, c, res, res, dtype=torch.float32, device=dev)
    out8 = torch.empty(n, res, res, c, dtype=torch.uint8, device=dev)
    lut_dev = image_io.normalize_table(3).to(dev)
    t_f32 = timed(lambda: ops.resample_u8(on_dev, recs, arena.buf, ws, out, n, c, res, res, max_rows, total_rows,
                                          lut=lut_dev), args.reps, args.inner)
    t_u8 = timed(lambda: ops.resample_u8(on_dev, recs, arena.buf, ws, out8, n, c, res, res, max_rows, total_rows),
                 args.reps, args.inner)
    # the public call from CPU tensors, host clock around a synchronise: pack into pinned memory, upload, two launches
    cpu_list = [torch.from_numpy(i) for i in images]

    def end_to_end():
        y = image_io.to_tensor(cpu_list, res, "lanczos", device=dev)
        torch.cuda.synchronize()
        return y

    assert torch.equal(end_to_end(), out)
    wall = float("inf")
    for _ in range(args.cpu_reps):
        t0 = time.perf_counter()
        end_to_end()
        wall = min(wall, time.perf_counter() - t0)
    # bytes from the shapes: the source rows pass 1 reads, the workspace, the output
    rows = []
    for h, _ in sizes:
        yb = image_io.resample_tables(h, res, "lanczos")[0] if h != res else None
        rows.append(h if yb is None else int(yb[-1, 0] + yb[-1, 1] - yb[0, 0]))
    assert sum(rows) == total_rows
    read_src = sum(r * w * c for r, (_, w) in zip(rows, sizes))
    ws_bytes = total_rows * res * c
    must_f32 = read_src + n * res * res * c * 4
    must_u8 = read_src + n * res * res * c

    # the CPU pipeline it replaces: PIL resize + the table, 16 threads, the same images (decoding excluded)
    pil = [Image.fromarray(i) for i in images]
    lut = image_io.normalize_table(3).numpy()
    ch = np.arange(3)

    def cpu_one(im):
        r = np.asarray(im.resize((res, res), Image.Resampling.LANCZOS))
        return np.ascontiguousarray(lut[ch, r].transpose(2, 0, 1))

    with ThreadPoolExecutor(args.threads) as pool:
        ref = list(pool.map(cpu_one, pil))   # warm-up, and the reference result
        best = float("inf")
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            list(pool.map(cpu_one, pil))
            best = min(best, time.perf_counter() - t0)
    assert np.array_equal(out.cpu().numpy().view(np.int32), np.stack(ref).view(np.int32)), "device != PIL + table"
    assert np.array_equal(out8.cpu().numpy(), np.stack([np.asarray(im.resize((res, res), Image.Resampling.LANCZOS))
                                                        for im in pil]))

    dev_per_img = (t_h2d[0] + t_f32[0]) * 1e-3 / n
    cpu_rate = n / best
    print(f"[{label}] {n} images, {src_bytes / 1e6:.1f} MB of uint8 sources -> {res} x {res}, LANCZOS; output equals "
          f"PIL + table bit for bit")
    print(f"  H2D of the sources (pinned)    {fmt(t_h2d)}  -> {src_bytes / (t_h2d[0] * 1e-3) / 1e9:.1f} GB/s")
    print(f"  to_tensor (2 launches, f32)    {fmt(t_f32)}  must move {must_f32 / 1e6:.1f} MB -> "
          f"{must_f32 / (t_f32[0] * 1e-3) / 1e12:.3f} TB/s = {must_f32 / (t_f32[0] * 1e-3) / HBM_PEAK * 100:.1f} % of "
          f"the 8.0 TB/s peak ({must_f32 / (t_f32[0] * 1e-3) / HBM_MEASURED * 100:.1f} % of the 6.29 TB/s copy rate)")
    print(f"  resize_u8 (2 launches, uint8)  {fmt(t_u8)}  must move {must_u8 / 1e6:.1f} MB -> "
          f"{must_u8 / (t_u8[0] * 1e-3) / 1e12:.3f} TB/s = {must_u8 / (t_u8[0] * 1e-3) / HBM_PEAK * 100:.1f} % of peak")
    print(f"  workspace, written and read once: 2 x {ws_bytes / 1e6:.1f} MB (not in the figures above)")
    print(f"  device path, upload + two launches (device events): {dev_per_img * 1e6:.1f} us per image = "
          f"{1 / dev_per_img:,.0f} img/s")
    print(f"  to_tensor(list of CPU tensors), host clock to synchronise (pinned pack + upload + launches): "
          f"{wall * 1e3:.2f} ms per {n} images = {n / wall:,.0f} img/s (best of {args.cpu_reps})")
    print(f"  CPU, PIL resize + table, {args.threads} threads: {best * 1e3:.1f} ms per {n} images = {cpu_rate:,.0f} "
          f"img/s (best of {args.cpu_reps})")
    for what, rate in (("upload + launches", 1 / dev_per_img), ("to_tensor from CPU tensors", n / wall)):
        verdict = "faster" if rate > cpu_rate else "NOT faster"
        print(f"  -> the device path ({what}) is {verdict} per image than the {args.threads}-thread CPU pipeline "
              f"({rate / cpu_rate:.1f} x)")


def to_uint8_workload(args, dev):
    from image_compression_2_amd import image_io
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.rand(32, 3, 256, 256, device=dev, generator=g) * 2.4 - 1.2
    must = x.numel() * 5
    print(f"[to_uint8] 32 x 3 x 256 x 256 f32 -> uint8 NHWC: must move {must / 1e6:.1f} MB (4 bytes read, 1 written)")
    for mode in ("eval", "save_image", "reference"):
        t = timed(lambda: image_io.to_uint8(x, mode), args.reps, args.inner)
        print(f"  {mode:11s} {fmt(t)}  -> {must / (t[0] * 1e-3) / 1e12:.3f} TB/s = "
              f"{must / (t[0] * 1e-3) / HBM_PEAK * 100:.1f} % of the 8.0 TB/s peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device {torch.cuda.get_device_name(0)}; Pillow {Image.__version__}; median (min .. max) of {args.reps} "
          f"batches of {args.inner} calls, device events")
    rng = np.random.default_rng(24)
    uniform = [rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8) for _ in range(32)]
    resample_workload("uniform 1024^2", uniform, 256, args, dev)
    sizes = rng.integers(300, 601, (32, 2))
    ragged = [rng.integers(0, 256, (int(h), int(w), 3), dtype=np.uint8) for h, w in sizes]
    resample_workload("ragged 300..600", ragged, 256, args, dev)
    to_uint8_workload(args, dev)


if __name__ == "__main__":
    main()
