"""TEST INFRASTRUCTURE -- fp64 CPU reference, per-element bound and case table of the filtered-lrelu FORWARD edge
tests (tests/test_gpu_flrelu_fwd_edges.py; pinned on the CPU by tests/test_flrelu_fwd_oracle_host.py).

Everything is plain fp64 torch on the CPU, built on ``oracle/sg3.py``.  The taps, the Gaussian input, the output
size, the padding tables and the layout helpers come from ``tests/flrelu_bwd_oracle.py``, so the forward and the
backward suites feed the same inputs.

``forward_reference`` takes the operands as the kernel stores them and returns NHWC fp64 tensors:

* ``ref``  sg3.filtered_lrelu(x, fu, fd, bias, ...) * post_scale[n, c];
* ``B``    the same chain on |x| + |bias|, |fu|, |fd| with slope 1 and no clamp, times |post_scale|.  Every product a
           correctly indexed kernel forms is one term of B, so each relative rounding it commits costs at most
           eps * B.  lrelu and the clamp are 1-Lipschitz and continuous: a perturbed pre-activation moves the
           activation by no more than itself, so the forward needs no mask allowance.

The bound, per output element:

    |got - ref| <= K * eps_op * B + eps_out * |ref| + F

eps_op   unit roundoff of the path's operands and intermediates: 2^-11 (f16) for both MFMA kernels (f16 taps, f16
         V / U / D images); 2^-24 for the f32 VALU instances; 2^-8 (bf16) for the bf16 VALU instances, whose LDS
         image holds packed bf16 pairs (flrelu_valu.h LdsPair<uint32_t>: the vertically up-sampled input and the
         horizontally down-sampled activation are both rounded to bf16).
eps_out  unit roundoff of the stored output (2^-8 bf16, 2^-11 f16, 2^-24 f32).
F        absolute floor of the MFMA paths for f16 intermediates below 2^-14 (subnormal: absolute error up to the
         half-spacing 2^-25 instead of a relative one).  Each stored intermediate contributes 2^-25 times the
         1-norms of the filters it still passes through (g1: the largest polyphase 1-norm of up * fu; d1: the 1-norm
         of fd), times gain and |post_scale|:
           V  (after the vertical up pass)        g1 * d1^2 * gain
           U  (after the horizontal up pass)      d1^2 * gain, times lim = clamp / gain on the clamp-split instances,
                                                  whose up pass produces u / lim
           D  (after the horizontal down pass)    d1
           x  (bf16 input below 2^-14 loses bits when converted to f16; tile kernel only)   g1^2 * d1^2 * gain
         plus 2^-25 for an f16 output.  Derived from the formats; nothing is fitted.

K, derived (count of roundings of relative size eps_op along the chain, read from the kernel source):

  strip / tile (MFMA)  14.  The four tap vectors (gu vertical, gu horizontal, gd * gain horizontal, gd vertical) are
      rounded jointly by f16_round_taps: every tap to one of its two f16 neighbours, up to 1 ulp = 2 eps each -> 8.
      The stored f16 images V, U and D -> 3.  The activation: the slope constant in f16 and the rounded product
      slope * u -> 2 (the clamp bound in f16 costs eps * lim <= eps * |u| where it acts and replaces the product's
      rounding there).  The f32 accumulations of 4 passes of at most 32 terms and the post_scale product, 2^-24
      each: 130 * 2^-13 eps < 1 -> 1.  The clamp-split instances (strip kernel, finite clamp with lim in [2^-4,
      2^12]) round gu / lim and gd * gain * lim instead of gu and gd * gain, the same count, except that the
      smallest up-4 tap over lim (4.2e-5 at clamp 256) lies in the first subnormal f16 binade [2^-15, 2^-14), where
      1 ulp is up to 4 eps: 16 for them.  The host test asserts that no scaled tap lies below 2^-15.
  valu f32             29.  FMA chains of 6 polyphase taps in each of the four passes (24), the bias add, the slope
      product, gain folded into the down taps, lim = clamp / gain, the post_scale product.
  valu bf16            2.1.  The two bf16 roundings of the LDS image; the 29 f32 roundings are 29 * 2^-16 eps_op.

The measured values and the bars live in tests/test_gpu_flrelu_fwd_edges.py and profiles/r19_flr_fwd_edges.txt.
"""
import numpy as np
import torch

import flrelu_bwd_oracle as fo
from oracle import sg3

GAIN = fo.GAIN
TIERS = fo.TIERS
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EPS_OUT = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}
# path -> bound key
KEY = {"strip": "mfma_strip", "tile": "mfma_tile", "valu16": "valu_bf16", "valu24": "valu_f32"}
EPS_OP = {"mfma_strip": 2.0 ** -11, "mfma_tile": 2.0 ** -11, "valu_f32": 2.0 ** -24, "valu_bf16": 2.0 ** -8}
K_DERIVED = {"mfma_strip": 14.0, "mfma_tile": 14.0, "valu_f32": 29.0, "valu_bf16": 2.1}
K_DERIVED_CLAMP_SPLIT = 16.0
C, C_P, N = fo.C, fo.C_P, fo.N
C_NCHW = 19


def key_of(path, xdt):
    if path == "nchw":
        return "valu_bf16" if xdt == BF16 else "valu_f32"
    return KEY[path]


# ------------------------------------------------------------------ the reference
def forward_reference(x, fu, fd, up, padding, gain=GAIN, slope=0.2, clamp=256.0, flip=False, bias=None,
                      post_scale=None, c=None):
    """x [n, h, w, c_p] as stored (any dtype); fu / fd taps; clamp < 0: none; bias [c_p] / post_scale [n, c_p] or
    None.  Returns a dict of NHWC fp64 tensors over the first `c` channels: ref, B; and the coverage figures of the
    activation grid: `clamped` [c] (share of grid positions per channel at the clamp) and `positive` (share of
    positions with a positive pre-activation)."""
    c = x.shape[-1] if c is None else c
    n = x.shape[0]
    fu, fd = fu.double(), fd.double()
    cl = None if clamp < 0 else float(clamp)
    xr = fo._nchw(x, c)
    bi = None if bias is None else bias.double()[:c]
    ps = torch.ones(n, c, dtype=torch.float64) if post_scale is None else post_scale.double()[:, :c]
    psb = ps[:, :, None, None]
    kw = dict(up=up, down=2, padding=padding, flip_filter=bool(flip))
    ref = sg3.filtered_lrelu(xr, fu, fd, bi, gain=gain, slope=slope, clamp=cl, **kw) * psb
    xa = xr.abs() + (0.0 if bi is None else bi.abs()[None, :, None, None])
    B = sg3.filtered_lrelu(xa, fu.abs(), fd.abs(), None, gain=gain, slope=1.0, clamp=None, **kw) * psb.abs()
    U = sg3.upfirdn2d(sg3.bias_act(xr, bi), fu, up=up, padding=padding, gain=up ** 2, flip_filter=bool(flip))
    act = torch.where(U > 0, U, U * slope) * gain
    clamped = (act.abs() >= cl).double().mean(dim=(0, 2, 3)) if cl is not None else torch.zeros(c, dtype=torch.float64)
    return dict(ref=fo._nhwc(ref), B=fo._nhwc(B), clamped=clamped, positive=(U > 0).double().mean().item())


def clamp_split(path, clamp, gain=GAIN):
    """True when the launch runs a clamp-split instance (flrelu_mfma.hip fm3_launch)."""
    lim = clamp / gain
    return path == "strip" and clamp >= 0 and 0.0625 <= lim <= 4096.0


def floor_f16(path, fu, fd, up, gain, clamp, post_scale, odt, xdt, n, c):
    """F of the module docstring -> [n, 1, 1, c] fp64 (0 on the VALU paths)."""
    if path not in ("strip", "tile"):
        return torch.zeros(n, 1, 1, c, dtype=torch.float64)
    g = fu.double().abs() * up
    g1 = max(g[p::up].sum().item() for p in range(up))
    d1 = fd.double().abs().sum().item()
    lim = clamp / gain if clamp_split(path, clamp, gain) else 1.0
    f0 = g1 * d1 * d1 * gain + lim * d1 * d1 * gain + d1
    if xdt == BF16:
        f0 += g1 * g1 * d1 * d1 * gain
    ps = torch.ones(n, c, dtype=torch.float64) if post_scale is None else post_scale.double()[:, :c].abs()
    return (2.0 ** -25 * f0 * ps + (2.0 ** -25 if odt == F16 else 0.0))[:, None, None, :]


def bound(r, K, eps_op, odt, F):
    return K * eps_op * r["B"] + EPS_OUT[odt] * r["ref"].abs() + F


# ------------------------------------------------------------------ f16_round_taps, restated (flrelu.hip)
def _f16_step(r, up_):
    h = np.float16(r)
    return np.float32(np.nextafter(h, np.float16(np.inf) if up_ else np.float16(-np.inf)))


def f16_round_taps(exact, groups):
    """exact: float32 taps -> f16-representable float32 taps; per group t mod `groups` every tap goes to one of its
    two f16 neighbours so that the group's sum error is minimal (greedy, as the library does it)."""
    exact = np.asarray(exact, dtype=np.float32)
    n = exact.shape[0]
    out = exact.astype(np.float16).astype(np.float32)
    for g in range(groups):
        idx = range(g, n, groups)
        for _ in range(n):
            e = sum(float(out[t]) - float(exact[t]) for t in idx)
            best, bi, bc = abs(e), -1, 0.0
            for t in idx:
                if exact[t] == 0:
                    continue
                for d in (True, False):
                    cnd = _f16_step(out[t], d)
                    if (float(cnd) - float(exact[t])) * (float(out[t]) - float(exact[t])) > 0:
                        continue
                    e2 = abs(e - float(out[t]) + float(cnd))
                    if e2 < best:
                        best, bi, bc = e2, t, cnd
            if bi < 0:
                break
            out[bi] = bc
    return out


def kernel_taps(fu, fd, up, gain, clamp, flip):
    """The f32 tap vectors of the MFMA launch, in correlation order, before and after the joint rounding:
    dict name -> (exact, rounded); gu (x up), gd, gdg (x gain), and for a finite clamp guh (gu / lim), gdgl."""
    gu = (fu if flip else fu.flip(0)).float().numpy() * np.float32(up)
    gd = (fd if flip else fd.flip(0)).float().numpy().copy()
    gdg = gd * np.float32(gain)
    t = {"gu": (gu, f16_round_taps(gu, up)), "gd": (gd, f16_round_taps(gd, 1)), "gdg": (gdg, f16_round_taps(gdg, 1))}
    if clamp >= 0:
        lim = np.float32(np.float32(clamp) / np.float32(gain))
        guh, gdgl = gu / lim, gdg * lim
        t["guh"] = (guh, f16_round_taps(guh, up))
        t["gdgl"] = (gdgl, f16_round_taps(gdgl, 1))
    return t


def _h(t):
    return t.to(F16).double()


def _corr(x, k, axis):
    """Valid correlation of x [n, c, h, w] (fp64) with the 1-D kernel k along `axis` (2: vertical, 3: horizontal)."""
    n, c, h, w = x.shape
    kk = torch.as_tensor(np.asarray(k, dtype=np.float64))
    kk = kk.reshape(1, 1, -1, 1) if axis == 2 else kk.reshape(1, 1, 1, -1)
    y = torch.nn.functional.conv2d(x.reshape(n * c, 1, h, w), kk)
    return y.reshape(n, c, y.shape[2], y.shape[3])


def emulate_f16_chain(x, fu, fd, up, padding, gain, slope, clamp, flip, post_scale, odt, split, c):
    """The MFMA kernels' arithmetic restated in torch: jointly rounded f16 taps, the V, U and D images rounded to f16,
    the f16 activation (plain, or clamp-split when `split`), accumulation in fp64 (the kernels': f32), the output
    rounded to `odt`.  -> NHWC fp64 [n, oh, ow, c]."""
    t = kernel_taps(fu, fd, up, gain, clamp, flip)
    xr = _h(fo._nchw(x, c))
    z = sg3.upfirdn2d(xr, torch.ones(1, 1, dtype=torch.float64), up=up, padding=padding)   # zero-insert, pad / crop
    V = _h(_corr(z, t["gu"][1], 2))
    sl = _h(torch.tensor(slope, dtype=torch.float32))
    if split:
        lim = float(np.float32(np.float32(clamp) / np.float32(gain)))
        assert 0.0625 <= lim <= 4096.0
        Us = _h(_corr(V, t["guh"][1], 3))
        act = Us.clamp(0, 1) - _h(-sl * Us).clamp(0, 1)
        D = _h(_corr(act, t["gdgl"][1], 3)[..., ::2])
    else:
        U = _h(_corr(V, t["gu"][1], 3))
        act = torch.maximum(U, _h(sl * U))
        if clamp >= 0:
            lim = _h(torch.tensor(float(np.float32(clamp) / np.float32(gain)), dtype=torch.float32))
            act = torch.minimum(torch.maximum(act, -lim), lim)
        D = _h(_corr(act, t["gdg"][1], 3)[..., ::2])
    O = _corr(D, t["gd"][1], 2)[:, :, ::2]
    if post_scale is not None:
        O = O * post_scale.float().double()[:, :c, None, None]
    return fo._nhwc(O.float().to(odt).double())


# ------------------------------------------------------------------ the case table
# name -> (up, [px0, px1, py0, py1]): the seven paddings of the backward sweep, up 4 at delta 0 and 1, and an up-2
# padding with px0 != py0 of the same phase.  delta = p0 mod up: (2,0) p10_9; (2,1) the other up-2 ones; (4,0)
# p16_13; (4,1) p13_16; (4,2) crop6_9, p14_15; (4,3) p15_14
PADS = {**{f"u2-{k}": (2, v) for k, v in fo.UP2_PADS.items()}, **{f"u4-{k}": (4, v) for k, v in fo.UP4_PADS.items()},
        "u4-p16_13": (4, [16, 13, 16, 13]), "u4-p13_16": (4, [13, 16, 13, 16]), "u2-p9_8_11_8": (2, [9, 8, 11, 8])}
# (out_h, out_w) targets per tile shape, non-square.  Strip (16 rows x 32 columns): widths 1, 31, 32, 33; heights
# whose last 16-row tile has 1, 11, 12, 16 live rows with one tile and with two (tail_skip acts at <= 11 live rows).
# 16 x 16 tiles (MFMA tile kernel, bf16 NHWC VALU): 15, 16, 17, 33 on both axes.  24 x 8 tiles (the other VALU
# instances): heights 23, 24, 25, widths 7, 8, 9, 17.
OUT_SIZES = {"strip": [(1, 31), (11, 33), (12, 1), (16, 32), (17, 33), (27, 1), (28, 32), (32, 31)],
             "tile": [(15, 16), (16, 17), (17, 33), (33, 15)],
             "valu16": [(15, 16), (16, 17), (17, 33), (33, 15)],
             "valu24": [(23, 7), (24, 8), (25, 9), (24, 17)],
             "nchw": [(23, 7), (24, 8), (25, 9), (24, 17)]}
PATHS = list(OUT_SIZES)


def reachable(target, up, p0, p1):
    """(in, out): the input size whose output is `target`.  Up 4 reaches even outputs only: an odd target t becomes
    t + 1 when t is one past a multiple of 8 (1, 17, 25, 33: the `one past a tile` cases stay past it) and t - 1
    otherwise (7, 11, 15, 23, 27, 31 stay short of it; 10 and 12 live rows still bracket tail_skip's 11)."""
    def find(t):
        for i in range(1, 400):
            if (i * up + p0 + p1 - 6 * up - 9) // 2 == t:
                return i
        return None
    i = find(target)
    if i is None:
        target = target + 1 if target % 8 == 1 else target - 1
        i = find(target)
    assert i is not None, (target, up, p0, p1)
    return i, target


def sweep_cases(path):
    """[dict(id, path, up, pad, in_h, in_w, flip, blocked_in, xdt)] of the geometry sweep of one path."""
    out = []
    for name, (up, pad) in PADS.items():
        if pad[0] < 0:
            sizes = fo.UP2_CROP_SIZES if up == 2 else fo.UP4_CROP_SIZES
        else:
            sizes = [(reachable(oh, up, pad[2], pad[3])[0], reachable(ow, up, pad[0], pad[1])[0])
                     for oh, ow in OUT_SIZES[path]]
        for h, w in sizes:
            i = len(out)
            xdt = {"strip": F16, "tile": BF16, "valu16": BF16, "valu24": F32}.get(path, (F32, BF16)[(i // 2) % 2])
            out.append(dict(id=f"{name}-{h}x{w}", path=path, up=up, pad=pad, in_h=h, in_w=w, flip=i % 2,
                            blocked_in=path == "strip" and (i // 2) % 2 == 1, xdt=xdt))
    return out


def mask_input(n, h, w, c, c_p, seed, dtype):
    """Gaussian x 3 with the first third of the channels x 100 (std 300: part of their grid clamps at 256)."""
    x = fo.gauss(n, h, w, c, c_p, seed, torch.float64, 3.0)
    x[..., : c // 3] *= 100.0
    return x.to(dtype)


def case_inputs(case, tier):
    """(x NHWC in the stored dtype, bias or None, post_scale or None, c) of one sweep case.  Bias only where the path
    takes one (the VALU kernel); post_scale (mixed signs) wherever the entry point takes one (not NCHW)."""
    path = case["path"]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"] + path)) % 100000
    c, c_p = (C_NCHW, C_NCHW) if path == "nchw" else (C, C_P)
    mk = mask_input if tier == "mask" else (lambda *a: fo.gauss(*a, 3.0))
    x = mk(N, case["in_h"], case["in_w"], c, c_p, seed, case["xdt"])
    ps, b = fo.scale_bias(N, c, c_p, seed + 2)
    return x, (b if path in ("valu16", "valu24", "nchw") else None), (None if path == "nchw" else ps), c


# matrix geometries (one per up factor) and the replicated cases
MATRIX = {2: ("u2-p9_8_9_10", 19, 35), 4: ("u4-p15_14", 17, 18)}   # (padding name, in_h, in_w): out 18 x 33 / 32 x 34

# chained strips: one sample of 16 channels, 17 columns wide (tiles_x = 1), replicated to n = 8 x c_p = 4096 by the GPU
# test: 2048 strips.  Heights of 3, 4, 5 tiles whose last tile has 11 (10 at up 4), 12, 16 live rows
CHAIN_N, CHAIN_CP, CHAIN_W = 8, 4096, 17
CHAIN_PAD = {2: [9, 8, 9, 8], 4: [15, 14, 15, 14]}
CHAIN_OUT_H = [43, 60, 80]
SCALES = [0.5, 1.0, 2.0, 4.0]
# persistent tile kernel: out 17 x 18 (up 2) / 18 x 18 (up 4) = 4 tiles x 128 channel blocks x n = 8 -> 4096 tiles
PERSIST_N, PERSIST_CP = 8, 2048
PERSIST = {2: ([9, 8, 9, 10], 18, 20), 4: ([15, 14, 15, 14], 10, 10)}   # (padding, in_h, in_w)


def chain_in_h(up, out_h):
    return reachable(out_h, up, CHAIN_PAD[up][2], CHAIN_PAD[up][3])


def scale_index(n, cblocks):
    """[n, cblocks] long: which of SCALES multiplies copy (sample, channel block).  Neighbouring samples and
    neighbouring blocks always differ, so a row fetched from the wrong one is off by at least 2 x."""
    s = torch.arange(n)[:, None]
    b = torch.arange(cblocks)[None, :]
    return (3 * s + b + b // 4) % 4


def replicated_inputs(up, tier, in_h, in_w, n, c_p, dtype, seed):
    """(x1 [1, h, w, 16] fp64 before scaling and rounding, post_scale [n, c_p] f32, idx [n, c_p / 16])."""
    mk = mask_input if tier == "mask" else (lambda *a: fo.gauss(*a, 3.0))
    x1 = mk(1, in_h, in_w, 16, 16, seed + up, dtype).double()   # rounded once: the power-of-two copies stay exact
    ps, _ = fo.scale_bias(n, c_p, c_p, seed + 11 + up)
    return x1, ps, scale_index(n, c_p // 16)


# ------------------------------------------------------------------ fm_strip_segments / fm_strip_grid, restated
def strip_segments(nstrips, tiles_y, resident, tune=True):
    nseg = (2 * resident + nstrips - 1) // nstrips
    nseg = max(1, min(nseg, tiles_y))
    if tune and tiles_y <= 40:
        best, pick = -1, nseg
        sg = nseg
        while sg <= tiles_y and sg <= nseg + 16:
            ln = (tiles_y + sg - 1) // sg
            segs = (tiles_y + ln - 1) // ln
            cost = (nstrips * segs + resident - 1) // resident * (ln + 1)
            if best < 0 or cost < best:
                best, pick = cost, segs
            sg += 1
        nseg = pick
    return nseg


def strip_grid(nstrips, tiles_y, resident, tune=True):
    seg_len = -(-tiles_y // strip_segments(nstrips, tiles_y, resident, tune))
    nseg = -(-tiles_y // seg_len)
    nitems = nstrips * nseg
    return dict(nseg=nseg, seg_len=seg_len, nitems=nitems, grid=min(nitems, resident))
