"""StyleGAN3-R-256 on the GPU: the f16 synthesis step at batch 8 and 32, and per radial layer shape the filtered lrelu
as the fused 2-D kernel (ic2_flrelu_nhwc16_2d, f16 -> f16) next to the unfused four-kernel composition
(sg3_ops.filtered_lrelu with the 2-D filter, NCHW bf16: bias_act / upfirdn2d / bias_act / upfirdn2d).  Device events
around warmed-up loops on random inputs; prints one JSON line.

    python tools/bench_sg3r.py [--batches 8,32] [--layers 0,3,8,10,11] [--layer-batch 8] [--reps 10]

Per layer: ms, the algorithmic bytes (input + output once, 2 B each) over the time, that over the HBM rate (8 TB/s
spec), and the FLOP/s of the 144-tap down FIR alone -- the bound that applies is the VALU one when the fraction of
the HBM floor is small.

    python tools/bench_sg3r.py --train [--layers 0,3,8,10,11] [--layer-batch 8] [--reps 7] [--out FILE]

Training through the R generator (Generator.set_radial_training).  Per layer shape the filtered lrelu's backward as the
fused kernel (ic2_flrelu_bwd_nhwc_2d: f16 x, bf16 gout and gx, oscale, bias and ydot set) against the composed
backward (autograd_ops._flrelu_backward_composed, all the code offered before the kernel), with the fused forward
beside it; then the synthesis forward + backward w.r.t. ws at batch 8 in bf16 and in f16 (train_f16, loss x 2^12).
Warm-up, then interleaved (fused, composed) pairs, each timed with device events; the medians are reported.  Every
step is a child process of its own under a time limit, run one after the other; the first that fails ends the run.
Prints one JSON line per step and the collected record last; --out appends them to a file."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_compression_2_amd as ic2  # noqa: E402
from image_compression_2_amd import sg3_ops  # noqa: E402

HBM_BPS = 8.0e12


def timed(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def layer_record(L, batch, reps, dev):
    s, so = int(L.in_size[0]) + L.conv_kernel - 1, int(L.out_size[0])
    g = torch.Generator(device=dev).manual_seed(3)
    y = (torch.randn(batch, L.cout_p // 16, s, s, 16, generator=g, device=dev) * 3).half()
    ps = torch.rand(batch, L.cout_p, generator=g, device=dev) + 0.5
    fused = lambda: L.flrelu_nhwc(y, torch.float16, ps, blocked=True, out_blocked=True)  # noqa: E731
    ms = timed(fused, reps)
    x = (torch.randn(batch, L.out_channels, s, s, generator=g, device=dev) * 3).bfloat16()
    fu, fd = L.up_filter.to(dev), L.down_filter.to(dev)
    comp = lambda: sg3_ops.filtered_lrelu(x, fu, fd, None, up=L.up_factor, down=L.down_factor,  # noqa: E731
                                          padding=L.padding, gain=np.sqrt(2), slope=0.2, clamp=256.0)
    ms_c = timed(comp, max(2, reps // 3))
    nbytes = 2 * batch * L.cout_p * (s * s + so * so)
    flops = 2 * 144 * batch * L.cout_p * so * so
    return {"shape": f"up{L.up_factor}_{s}->{so}_c{L.cout_p}", "rank": L.down_rank, "fused_ms": round(ms, 4),
            "composition_ms": round(ms_c, 4), "alg_bytes": nbytes, "alg_TBps": round(nbytes / ms / 1e9, 3),
            "hbm_floor_fraction": round(nbytes / HBM_BPS / (ms * 1e-3), 4),
            "down_fir_TFLOPs": round(flops / ms / 1e9, 2)}


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def paired_medians(fns, reps, warmup=2):
    """Medians of the calls' times over `reps` interleaved rounds (one call of each per round) after `warmup` rounds."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ms[k].append(_event_ms(fn))
    return [float(np.median(v)) for v in ms]


def train_layer_record(L, batch, reps, dev):
    """Fused backward, composed backward and fused forward of one radial layer's filtered lrelu (bf16 training dtypes)."""
    import ctypes
    from image_compression_2_amd import _native as nv
    from image_compression_2_amd import autograd_ops as ao
    s, so = int(L.in_size[0]) + L.conv_kernel - 1, int(L.out_size[0])
    c_p = L.cout_p
    g = torch.Generator(device=dev).manual_seed(3)
    y = (torch.randn(batch, s, s, c_p, generator=g, device=dev) * 3).half()
    dout = torch.randn(batch, so, so, c_p, generator=g, device=dev).bfloat16()
    os_ = torch.rand(batch, c_p, generator=g, device=dev) + 0.5
    bias = torch.randn(c_p, generator=g, device=dev)
    dc = torch.empty_like(y, dtype=torch.bfloat16)
    nyd = int(nv.query("ic2_flrelu_bwd_2d_ydot_floats", batch, c_p, s, s, L.up_factor))
    ydot = torch.empty([nyd], dtype=torch.float32, device=dev)
    fu, fd = L._fu, L._fd
    clamp = float(L.conv_clamp) if L.conv_clamp is not None else -1.0

    def fused():
        nv.call("ic2_flrelu_bwd_nhwc_2d", nv.ptr(y), nv.F16, nv.ptr(dout), nv.BF16, nv.ptr(dc), nv.BF16, batch, c_p, s, s,
                so, so, fu.ctypes.data_as(ctypes.c_void_p), fu.shape[0], fd.ctypes.data_as(ctypes.c_void_p), fd.shape[0],
                L.up_factor, L.down_factor, *L.padding, float(L.act_gain), 0.2, clamp, 0, nv.ptr(os_), nv.ptr(bias),
                nv.ptr(ydot), nyd, nv.stream_of(y))

    composed = lambda: ao._flrelu_backward_composed(y, dout, L)  # noqa: E731
    forward = lambda: L.flrelu_nhwc(y, torch.bfloat16, os_)      # noqa: E731
    ms_f, ms_c, ms_fwd = paired_medians([fused, composed, forward], reps)
    return {"shape": f"up{L.up_factor}_{s}->{so}_c{c_p}", "batch": batch, "bwd_fused_ms": round(ms_f, 4),
            "bwd_composed_ms": round(ms_c, 4), "composed_over_fused": round(ms_c / ms_f, 2),
            "fwd_fused_ms": round(ms_fwd, 4), "bwd_over_fwd": round(ms_f / ms_fwd, 2),
            "gather_TFLOPs": round(2 * 36 * batch * c_p * (2 * so + 11) ** 2 / ms_f / 1e9, 2)}


def train_synthesis_record(precision, batch, reps, dev):
    """R-256 synthesis forward + backward w.r.t. ws (bf16, or f16 with train_f16 and the loss scaled by 2^12)."""
    G = ic2.make_generator(256, seed=1, precision=precision, device=dev, **ic2.SG3_R_KWARGS).set_radial_training()
    G.synthesis.train_f16 = precision == "f16"
    scale = 4096.0 if precision == "f16" else 1.0
    ws = torch.randn(batch, G.num_ws, G.w_dim, generator=torch.Generator().manual_seed(2)).to(dev).requires_grad_(True)
    r = torch.randn(batch, 3, 256, 256, generator=torch.Generator().manual_seed(4)).to(dev) * scale
    fin = []

    def step():
        ws.grad = None
        (G.synthesis(ws) * r).sum().backward()
        fin.append(bool(torch.isfinite(ws.grad).all()))

    def fwd():
        with torch.no_grad():
            G.synthesis(ws)

    ms, ms_fwd = paired_medians([step, fwd], reps)
    return {"precision": precision, "batch": batch, "rounds": reps, "warmup_rounds": 2, "fwd_bwd_ms": round(ms, 3), "nograd_fwd_ms": round(ms_fwd, 3),
            "img_per_s": round(batch / ms * 1e3, 1), "grad_finite": all(fin)}


def train_step_main(a, dev):
    """One --train step in this process: layer:<index> or synthesis:<precision>."""
    kind, what = a.train_step.split(":")
    if kind == "layer":
        G = ic2.make_generator(256, seed=1, precision="bf16", device=dev, **ic2.SG3_R_KWARGS)
        i = int(what)
        rec = {"step": a.train_step, "layer": G.synthesis.layer_names[i]}
        rec.update(train_layer_record(G.synthesis.layers()[i], a.layer_batch, a.reps, dev))
    else:
        rec = {"step": a.train_step}
        rec.update(train_synthesis_record(what, a.layer_batch, a.reps, dev))
    print(json.dumps(rec))


def train_main(a):
    """The --train driver: never opens the GPU itself; one child per step under its own time limit, in order."""
    steps = [f"layer:{int(v)}" for v in a.layers.split(",") if v] + ["synthesis:bf16", "synthesis:f16"]
    out = {"generator": "stylegan3-r-256", "mode": "train", "steps": []}
    for st in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--train-step", st, "--layer-batch", str(a.layer_batch),
               "--reps", str(a.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            out["failed"] = f"{st}: over its {a.step_timeout} s limit"
            break
        if p.returncode != 0:
            out["failed"] = f"{st}: exit {p.returncode}: {p.stderr[-400:]}"
            break
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        out["steps"].append(json.loads(line))
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    print(json.dumps(out))
    return 1 if "failed" in out else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--layers", default="0,3,8,10,11")
    ap.add_argument("--layer-batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 7 if (a.train or a.train_step) else 10
    if a.train:
        raise SystemExit(train_main(a))
    if a.train_step:
        if not torch.cuda.is_available():
            raise SystemExit("bench_sg3r: needs a ROCm GPU (no CPU timing)")
        return train_step_main(a, torch.device("cuda", 0))
    if not torch.cuda.is_available():
        raise SystemExit("bench_sg3r: needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    G = ic2.make_generator(256, seed=1, precision="f16", device=dev, **ic2.SG3_R_KWARGS)
    out = {"generator": "stylegan3-r-256", "precision": "f16", "synthesis": {}, "layers": {}}
    with torch.no_grad():
        for b in [int(v) for v in a.batches.split(",") if v]:
            ws = torch.randn(b, G.num_ws, G.w_dim, generator=torch.Generator().manual_seed(2)).to(dev)
            ms = timed(lambda: G.synthesis(ws), a.reps)
            out["synthesis"][f"batch{b}"] = {"ms_per_step": round(ms, 3), "img_per_s": round(b / ms * 1e3, 1)}
        layers = G.synthesis.layers()
        for i in [int(v) for v in a.layers.split(",") if v]:
            out["layers"][G.synthesis.layer_names[i]] = layer_record(layers[i], a.layer_batch, a.reps, dev)
    out["layers_fused_ms_sum"] = round(sum(r["fused_ms"] for r in out["layers"].values()), 4)
    out["layers_composition_ms_sum"] = round(sum(r["composition_ms"] for r in out["layers"].values()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
