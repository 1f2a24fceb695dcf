"""Generates tests/golden/conv_plan_table.npz: what the conv launch planner answers over a grid of geometries.

Host only (the four plan queries of libic2ops.so run without a GPU; under a second).  The table pins the whole decision
surface of the planner -- kernel family, tile instance, split-K / tail / 384 forms, workspace bytes, channel-blocked
input acceptance, fused GroupNorm statistics -- so that a change to the dispatcher which is meant to keep the plan can
be checked row by row (tests/test_conv_plan_table.py re-runs sweep() and compares).  Regenerate it only with a change
that is meant to alter the plan, and say so in that change.

Grid (grid() below; rows with more than 3 * 2^31 input elements are left out, the ones between 2^31 and that cap keep
the 2 GiB chunking path covered):
  dtype      F32, BF16, F16 (cin_p = cin); BF16X3 (cin_p = 3 cin); F16X2 (cin_p = 2 cin)
  h = w      4 8 16 31 36 47 52 64 84 148 256 276 532 1024
  cin        32 64 96 128 256 512
  cout       (cout_p, cout_valid): (32,3) (32,32) (64,64) (96,96) (128,128) (192,181) (256,256) (384,362) (512,512)
  kernel     (kh, kw, pad): (3,3,1) (3,3,2) (1,1,0)
  n          1 8 32
  output     split dtypes: (F32, NHWC); plain dtypes: (dtype, NHWC), (F32, NCHW) and, for BF16 / F16, (dtype, NHWC16)
Per row: ic2_conv_plan (an index into `names`), ic2_conv_igemm_ws_bytes, ic2_conv_accepts_nhwc16 and, for the 3x3 pad-1
rows, ic2_conv3x3_gn_fuses(groups = 32, fuse = -1) (-1 elsewhere).

The knobs must be off (no IC2_DEV=1): run it from a clean environment.

    python tests/golden/make_conv_plan_table.py [--out PATH]
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv_plan_table.npz")

F32, BF16, F16, BF16X3, F16X2 = 0, 1, 2, 3, 4
NHWC, NCHW, NHWC16 = 0, 1, 2
DTYPES = ((F32, 1), (BF16, 1), (F16, 1), (BF16X3, 3), (F16X2, 2))  # (dtype, K multiplier)
SIZES = (4, 8, 16, 31, 36, 47, 52, 64, 84, 148, 256, 276, 532, 1024)
CINS = (32, 64, 96, 128, 256, 512)
COUTS = ((32, 3), (32, 32), (64, 64), (96, 96), (128, 128), (192, 181), (256, 256), (384, 362), (512, 512))
KERNELS = ((3, 3, 1), (3, 3, 2), (1, 1, 0))
BATCHES = (1, 8, 32)
MAX_X_ELEMS = 3 * 2 ** 31
COLUMNS = ("dtype", "out_dtype", "out_layout", "n", "h", "w", "cin_p", "cout_p", "cout_valid", "kh", "kw", "pad")


def outputs_of(dtype):
    if dtype in (BF16X3, F16X2):
        return ((F32, NHWC),)
    out = [(dtype, NHWC), (F32, NCHW)]
    if dtype in (BF16, F16):
        out.append((dtype, NHWC16))
    return tuple(out)


def grid():
    """The geometries, one row per COLUMNS tuple, int64 [rows, 12]."""
    rows = []
    for dtype, kmul in DTYPES:
        for hw in SIZES:
            for cin in CINS:
                cin_p = cin * kmul
                for cout_p, cout_valid in COUTS:
                    for kh, kw, pad in KERNELS:
                        for n in BATCHES:
                            if n * hw * hw * cin_p > MAX_X_ELEMS:
                                continue
                            for out_dtype, layout in outputs_of(dtype):
                                rows.append((dtype, out_dtype, layout, n, hw, hw, cin_p, cout_p, cout_valid, kh, kw, pad))
    return np.asarray(rows, dtype=np.int64)


def sweep():
    """The planner's answers over grid(): dict(geom, names, name_idx, ws_bytes, nhwc16, gn_fuses)."""
    from image_compression_2_amd import _native as nv
    if nv.query("ic2_dev_mode"):
        raise RuntimeError("the plan table is taken with the development knobs off (unset IC2_DEV)")
    lib = nv.load()
    geom = grid()
    plans, ws, blocked, gn = [], [], [], []
    for dtype, out_dtype, layout, n, h, w, cin_p, cout_p, cout_valid, kh, kw, pad in geom.tolist():
        plans.append(lib.ic2_conv_plan(dtype, out_dtype, layout, n, h, w, cin_p, cout_p, cout_valid, kh, kw, pad).decode())
        ws.append(lib.ic2_conv_igemm_ws_bytes(dtype, n, h, w, cin_p, cout_p, kh, kw, pad))
        blocked.append(lib.ic2_conv_accepts_nhwc16(dtype, out_dtype, layout, n, h, w, cin_p, cout_p, cout_valid, kh, kw,
                                                   pad))
        gn.append(lib.ic2_conv3x3_gn_fuses(dtype, n, h, w, cin_p, cout_p, cout_valid, kh, kw, pad, 32, -1)
                  if (kh, kw, pad) == (3, 3, 1) else -1)
    names = sorted(set(plans))
    index = {s: i for i, s in enumerate(names)}
    return {"geom": geom.astype(np.int32), "names": np.asarray(names),
            "name_idx": np.asarray([index[s] for s in plans], dtype=np.uint8),
            "ws_bytes": np.asarray(ws, dtype=np.int64), "nhwc16": np.asarray(blocked, dtype=np.int8),
            "gn_fuses": np.asarray(gn, dtype=np.int8)}


def main():
    out = OUT
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    t = sweep()
    np.savez_compressed(out, **{k: v for k, v in t.items() if k != "geom"})  # the rows are grid()'s, in its order
    print(f"[conv_plan_table] {len(t['name_idx'])} rows, {len(t['names'])} plan names, "
          f"{int((t['ws_bytes'] > 0).sum())} with a workspace, {int((t['nhwc16'] == 1).sum())} accept NHWC16, "
          f"{int((t['gn_fuses'] == 1).sum())} fuse the GroupNorm statistics")
    print(f"[conv_plan_table] wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
