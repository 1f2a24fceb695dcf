"""StyleGAN3-R-256 on the GPU: the f16 synthesis step at batch 8 and 32, and per radial layer shape the filtered lrelu
as the fused 2-D kernel (ic2_flrelu_nhwc16_2d, f16 -> f16) next to the unfused four-kernel composition
(sg3_ops.filtered_lrelu with the 2-D filter, NCHW bf16: bias_act / upfirdn2d / bias_act / upfirdn2d).  Device events
around warmed-up loops on random inputs; prints one JSON line.

    python tools/bench_sg3r.py [--batches 8,32] [--layers 0,3,8,10,11] [--layer-batch 8] [--reps 10]

Per layer: ms, the algorithmic bytes (input + output once, 2 B each) over the time, that over the HBM rate (8 TB/s
spec), and the FLOP/s of the 144-tap down FIR alone -- the bound that applies is the VALU one when the fraction of
the HBM floor is small."""
import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--layers", default="0,3,8,10,11")
    ap.add_argument("--layer-batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
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
