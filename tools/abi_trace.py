#!/usr/bin/env python
"""Record what the Python layer asks of libic2ops, to compare two trees (a refactor of the Python side must leave it
unchanged).  It hooks `_native` only: `_native._lib` becomes a recording proxy around the loaded library and
`_native._flops_hook` records the announced FLOPs.  Per scenario it writes, in order, every native call's name with
every non-pointer argument by value and each pointer argument as null / ptr, each announced FLOPs value, and a SHA-256
of every output tensor and gradient.

    python tools/abi_trace.py --out trace.json [--only encoder,synthesis,radial,train,composed]   (needs the GPU)
    python tools/abi_trace.py --diff a.json b.json      -> per-scenario summary of both and the first difference
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SMALL = dict(z_dim=32, w_dim=32, img_resolution=32, num_layers=6, channel_base=256, channel_max=24)


class Recorder:
    """Proxy around the CDLL: every function but ic2_last_error is recorded, then forwarded."""

    def __init__(self, nv, lib):
        self._nv, self._lib, self.events = nv, lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "ic2_last_error":
            return fn
        types = self._nv._SIGS[name]

        def wrapped(*args):
            rec = []
            for a, t in zip(args, types):
                if t is ctypes.c_void_p:
                    null = a is None or (isinstance(a, ctypes.c_void_p) and not a.value) or a == 0
                    rec.append("null" if null else "ptr")
                else:
                    rec.append(repr(float(a)) if t is ctypes.c_float else int(a))
            rc = fn(*args)
            self.events.append([name, rec, rc.decode() if isinstance(rc, bytes) else int(rc)])
            return rc
        return wrapped

    def flops(self, f):
        self.events.append(["note_flops", [int(f)], 0])


def sha(t):
    import torch
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def seed(s):
    import torch
    torch.manual_seed(s)
    torch.cuda.manual_seed_all(s)


def scenarios(only):
    import torch
    import image_compression_2_amd as ic2
    from image_compression_2_amd import _native as nv
    from image_compression_2_amd import autograd_ops as ao
    from image_compression_2_amd import networks_stylegan3 as ns
    from image_compression_2_amd import training
    dev = torch.device("cuda")
    lib = nv.load()
    out = {}

    def run(name, fn):
        rec = Recorder(nv, lib)
        nv._lib, nv._flops_hook = rec, rec.flops
        try:
            tensors = fn()
        finally:
            nv._lib, nv._flops_hook = lib, None
        torch.cuda.synchronize()
        out[name] = {"events": rec.events, "sha": [sha(t) for t in tensors]}
        print(f"[abi_trace] {name}: {len(rec.events)} events, {len(tensors)} tensors", flush=True)

    def encoder(w_dim):
        seed(0)
        return ic2.HVAE_VGG_Encoder(img_resolution=64, channel_base=256, channel_max=32, w_dim=w_dim).to(dev)

    def images():
        return (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)

    if "encoder" in only:
        enc = encoder(32).eval().requires_grad_(False)
        x = images()
        for prec in ("fp32", "bf16", "bf16x3", "f16"):
            def fn(prec=prec):
                enc.set_precision(prec)
                seed(1)
                with torch.no_grad():
                    return list(enc(x))
            run(f"encoder/{prec}", fn)

    if "synthesis" in only or "train" in only:
        seed(5)
        G = ns.Generator(img_resolution=256).to(dev).eval().requires_grad_(False)
    if "synthesis" in only:
        ws = torch.randn(2, 16, 512, generator=torch.Generator().manual_seed(4)).to(dev)
        saved = ns._ACT_BLOCKED, ns._SYNTH_TRIM
        for handoff in (True, False):
            ns._ACT_BLOCKED, ns._SYNTH_TRIM = (saved if handoff else (False, False))
            for prec in ("fp32", "bf16", "f16"):
                def fn(prec=prec):
                    G.set_precision(prec)
                    G.synthesis.__dict__.pop("_trim_plans", None)
                    with torch.no_grad():
                        return [G.synthesis(ws)]
                run(f"synthesis/{prec}/{'handoff' if handoff else 'plain'}", fn)
        ns._ACT_BLOCKED, ns._SYNTH_TRIM = saved
        G.synthesis.__dict__.pop("_trim_plans", None)

    if "radial" in only:
        seed(6)
        R = ns.Generator(**SMALL, conv_kernel=1, use_radial_filters=True).to(dev).eval().requires_grad_(False)
        R.set_radial_training()
        wr = torch.randn(2, R.num_ws, 32, generator=torch.Generator().manual_seed(7)).to(dev)

        def fn():
            w = wr.clone().requires_grad_(True)
            img = R.synthesis(w)
            img.backward(torch.ones_like(img))
            return [img, w.grad]
        run("radial/fp32", fn)

    if "train" in only:
        for prec in ("fp32", "bf16", "f16"):
            def fn(prec=prec):
                enc = encoder(512)   # W+ must be as wide as the 256 generator's
                enc.set_precision(prec)
                G.set_precision(prec)
                G.synthesis.train_f16 = False
                comp = ic2.StyleGAN3Compressor(enc, G, training_resolution=64)
                scaler = training.make_f16(comp) if prec == "f16" else None
                opt = training.make_optimizer(enc)
                seed(2)
                losses = training.train_step(comp, images(), opt, G.mapping.w_avg.view(1, 1, -1), perceptual_weight=0.0,
                                             scaler=scaler)
                G.synthesis.train_f16 = False
                return [losses[k].float() for k in sorted(losses)] + [p.grad for p in enc.parameters() if p.grad is not None]
            run(f"train/{prec}", fn)

    if "composed" in only:
        # a StyleGAN3-T layer whose padding is shifted by `up` between the axes (same output size): the forward runs the
        # fused kernel (px0 == py0 mod up), the backward has px0 != py0 and composes (autograd_ops._flrelu_backward_composed)
        seed(8)
        T = ns.Generator(**SMALL).to(dev).eval().requires_grad_(False)
        L = next(L for L in T.synthesis.layers() if not L.is_torgb and not L.is_critically_sampled and L.up_factor == 2)
        px0, px1, py0, py1 = L.padding
        L.padding = [px0 + L.up_factor, px1 - L.up_factor, py0, py1]
        g = torch.Generator().manual_seed(9)
        s_in = int(L.in_size[0])
        x0 = torch.randn(2, s_in, s_in, L.cin_p, generator=g).to(dev)
        xs0 = (torch.rand(2, L.cin_p, generator=g) + 0.5).to(dev)
        os0 = (torch.rand(2, L.cout_p, generator=g) + 0.5).to(dev)
        y0 = torch.randn(2, s_in + L.conv_kernel - 1, s_in + L.conv_kernel - 1, L.cout_p, generator=g).to(dev)

        def layer():
            x, xs, os_ = (t.clone().requires_grad_(True) for t in (x0, xs0, os0))
            o = ao.SynthLayerNHWC.apply(x, xs, os_, L, torch.float32)
            o.backward(torch.ones_like(o))
            return [o, x.grad, xs.grad, os_.grad]
        run("composed/SynthLayerNHWC", layer)

        def flr():
            y = y0.clone().requires_grad_(True)
            o = ao.FilteredLReluNHWC.apply(y, L, torch.float32)
            o.backward(torch.ones_like(o))
            return [o, y.grad]
        run("composed/FilteredLReluNHWC", flr)
    return out


def summary(tr):
    lines = []
    for name in sorted(tr):
        ev = tr[name]["events"]
        calls = [e for e in ev if e[0] != "note_flops"]
        fl = sum(e[1][0] for e in ev if e[0] == "note_flops")
        h = hashlib.sha256(json.dumps([ev, tr[name]["sha"]]).encode()).hexdigest()[:16]
        lines.append(f"  {name:36s} {len(calls):5d} calls  {len(ev) - len(calls):3d} flops notes (sum {fl})  "
                     f"{len(tr[name]['sha']):3d} tensors  digest {h}")
    return lines


def diff(a, b):
    bad = []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            bad.append(f"  {name}: only in {'A' if name in a else 'B'}")
            continue
        ea, eb = a[name]["events"], b[name]["events"]
        for i, (x, y) in enumerate(zip(ea, eb)):
            if x != y:
                bad.append(f"  {name}: event {i} differs\n    A {x}\n    B {y}")
                break
        else:
            if len(ea) != len(eb):
                bad.append(f"  {name}: {len(ea)} events in A, {len(eb)} in B")
        if a[name]["sha"] != b[name]["sha"]:
            n = sum(x != y for x, y in zip(a[name]["sha"], b[name]["sha"])) + abs(len(a[name]["sha"]) - len(b[name]["sha"]))
            bad.append(f"  {name}: {n} tensor hash(es) differ")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", default="encoder,synthesis,radial,train,composed")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.diff:
        a, b = (json.load(open(p)) for p in args.diff)
        print(f"A = {args.diff[0]}")
        print("\n".join(summary(a)))
        print(f"B = {args.diff[1]}")
        print("\n".join(summary(b)))
        bad = diff(a, b)
        print("DIFFERENCES:\n" + "\n".join(bad) if bad else
              f"IDENTICAL: {len(a)} scenarios, every event and every tensor hash equal")
        return 1 if bad else 0
    tr = scenarios(set(args.only.split(",")))
    with open(args.out, "w") as f:
        json.dump(tr, f)
    print("\n".join(summary(tr)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
