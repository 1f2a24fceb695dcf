"""TEST INFRASTRUCTURE -- fp64 CPU reference of the filtered-lrelu backward, for the per-element edge tests.

Everything is plain fp64 torch on the CPU, built on ``oracle/sg3.py`` (``upfirdn2d`` / ``filtered_lrelu``) and its
autograd.  ``reference`` takes the operands as the kernel stores them (x and gout already rounded to their storage
dtype) and returns, per element of x:

* ``ref``   dL/dx * oscale, by autograd through ``sg3.filtered_lrelu``;
* ``ydot``  sum over pixels of (dL/dx) * (x - bias), per sample and channel (``ref0`` is the unscaled dL/dx);
* ``B``     the magnitude bound: the same chain on |taps| and |gout| with slope 1 and no clamp, times |oscale|.  Every
            product a correctly indexed kernel forms is one term of B, so its rounding error is proportional to B;
* ``A``     the mask allowance.  U is the upsampled pre-activation, Ua the same from |x| and |fu|.  A grid position
            is fragile when a perturbation dU = kappa * eps_x * Ua of U (eps_x: the unit roundoff of the kernel's
            recompute of U) can change its lrelu side (|U| < dU) or its clamp decision (|gain * lrelu(U)| within
            gain * dU of the clamp).  A flipped decision changes the local gradient by at most w * gain * gD, with gD
            = |fd|^T |gout| the adjoint down FIR of |gout| on the U grid and w = 1 - slope (lrelu side) or the slope
            of the branch (clamp side: 1 for U > 0).  A = |oscale| * |fu|^T (fragile * gain * w * gD).

The builders below (taps, inputs, geometries) are shared by the GPU tests and the host test that pins this helper,
so the host test checks the very inputs the GPU cases run.
"""
import math

import torch

from oracle import sg3

GAIN = math.sqrt(2.0)
KAPPA = 4.0
EPS_X = {"mfma": 2.0 ** -11, "valu": 2.0 ** -24}   # U recompute: f16 operands / f32 arithmetic
TIERS = {"linear": dict(slope=1.0, clamp=-1.0), "mask": dict(slope=0.2, clamp=256.0)}


# ------------------------------------------------------------------ builders
def out_size(in_h, in_w, up, padding):
    tu, td = 6 * up, 12
    return sg3.filtered_lrelu_out_size(in_h, in_w, tu, td, up, 2, padding)


def taps(up, asym=True):
    """(fu, fd) float32: the SG3 low-pass design; asymmetric = times a linear ramp (a different one per filter),
    renormalised to sum 1, so a reversed tap order changes the result."""
    fu = sg3.design_lowpass_filter(6 * up, 8.0, 4.0, 64).double()
    fd = sg3.design_lowpass_filter(12, 8.0, 4.0, 64).double()
    if asym:
        fu = fu * torch.linspace(0.4, 1.6, fu.numel(), dtype=torch.float64)
        fd = fd * torch.linspace(1.5, 0.5, fd.numel(), dtype=torch.float64)
        fu, fd = fu / fu.sum(), fd / fd.sum()
    return fu.float().contiguous(), fd.float().contiguous()


def block_sign_input(n, h, w, c, c_p, seed, dtype, big=40.0, block=8):
    """NHWC [n, h, w, c_p] in `dtype`: per channel block x block pixel blocks of random sign times 4 + 2 |N(0,1)|
    (drawn per pixel), the first third of the channels times `big` (their positive blocks clamp at 256 / sqrt 2);
    channels [c, c_p) are 0.  Few grid positions sit near 0 or near the clamp, which keeps the mask allowance A off
    most elements."""
    g = torch.Generator().manual_seed(seed)
    bh, bw = (h + block - 1) // block, (w + block - 1) // block
    sign = (torch.randint(0, 2, (n, bh, bw, c), generator=g) * 2 - 1).double()
    sign = sign.repeat_interleave(block, 1).repeat_interleave(block, 2)[:, :h, :w]
    x = sign * (4.0 + 2.0 * torch.randn(n, h, w, c, generator=g, dtype=torch.float64).abs())
    x[..., : c // 3] *= big
    out = torch.zeros(n, h, w, c_p, dtype=torch.float64)
    out[..., :c] = x
    return out.to(dtype)


def gauss(n, h, w, c, c_p, seed, dtype, scale=1.0):
    """NHWC [n, h, w, c_p] in `dtype`: N(0, scale^2) on the valid channels, 0 on [c, c_p)."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(n, h, w, c_p, dtype=torch.float64)
    out[..., :c] = torch.randn(n, h, w, c, generator=g, dtype=torch.float64) * scale
    return out.to(dtype)


def scale_bias(n, c, c_p, seed):
    """(oscale [n, c_p], bias [c_p]) float32, 0 on the padded channels; oscale in +-[0.5, 1.5] with mixed signs."""
    g = torch.Generator().manual_seed(seed)
    os_ = torch.zeros(n, c_p)
    os_[:, :c] = (torch.rand(n, c, generator=g) + 0.5) * (torch.randint(0, 2, (n, c), generator=g) * 2 - 1).float()
    b = torch.zeros(c_p)
    b[:c] = torch.randn(c, generator=g)
    return os_, b


# up 2: 12 / 12 taps.  out = in - 2 ([9,8]), in - 1 ([10,9]), (in - 1) x (in - 2) ([9,8,9,10]), in - 22 (the crop)
UP2_PADS = {"p9_8": [9, 8, 9, 8], "p10_9": [10, 9, 10, 9], "p9_8_9_10": [9, 8, 9, 10], "crop11_12": [-11, -12, -11, -12]}
# up 4: 24 / 12 taps.  out = 2 in - 24 (the crop), 2 in - 2 (both positive paddings)
UP4_PADS = {"crop6_9": [-6, -9, -6, -9], "p15_14": [15, 14, 15, 14], "p14_15": [14, 15, 14, 15]}
# (in_h, in_w): every listed side once per padding, in_h != in_w; single partial tile (5), one short of / exactly /
# one past a 16-row tile (15, 16, 17) and of an 8 / 16-column strip (7, 8, 9 / 15, 16, 17), two tiles +-1 (31, 33)
UP2_SIZES = [(5, 7), (15, 16), (16, 15), (17, 33), (31, 17), (33, 16)]
UP4_SIZES = [(5, 3), (15, 7), (16, 8), (17, 9), (31, 17), (33, 21)]
# the crops need in >= 23 (up 2) / in >= 13 (up 4) per side.  Of the listed up-2 widths only 33 is wide enough and
# in_h != in_w, so the second up-2 crop takes width 23, the narrowest with an output (one column)
UP2_CROP_SIZES = [(31, 33), (33, 23)]
UP4_CROP_SIZES = [(15, 17), (16, 21), (17, 21), (31, 17), (33, 21)]


def geometries():
    """[(id, up, padding, in_h, in_w)] of the edge sweep."""
    out = []
    for name, pad in UP2_PADS.items():
        for h, w in (UP2_CROP_SIZES if pad[0] < 0 else UP2_SIZES):
            out.append((f"u2-{name}-{h}x{w}", 2, pad, h, w))
    for name, pad in UP4_PADS.items():
        for h, w in (UP4_CROP_SIZES if pad[0] < 0 else UP4_SIZES):
            out.append((f"u4-{name}-{h}x{w}", 4, pad, h, w))
    return out


C, C_P, N = 22, 32, 2   # valid / padded channels and samples of the sweep
# (big, block) of the mask tier's block-sign input.  Up 2: 8x8 blocks, clamp channels x 40.  At up 4 one fragile grid
# position reaches 6 x 6 elements of gx and x 40 leaves a fifth of the positive pixels (160 .. 181) under the clamp, so
# U keeps crossing it inside the blocks: with that input 21 .. 33 % of the elements carry an allowance at the positive
# up-4 paddings (f16 recompute), over the 20 % the tier allows.  x 64 puts every positive pixel (>= 256) over the clamp
# and 12 x 12 blocks thin the sign changes; the worst up-4 case is then 16 %.
MASK_INPUT = {2: (40.0, 8), 4: (64.0, 12)}


def case_inputs(gid, up, padding, in_h, in_w, path, tier, gscale=1.0, c=C, c_p=C_P, n=N):
    """The stored operands of one sweep case: x (f16 on the MFMA path, f32 on the VALU path), gout (bf16 / f32),
    oscale, bias.  Linear tier: Gaussian x (no mask decision exists); mask tier: block-sign x."""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(gid)) % 100000
    xdt = torch.float16 if path == "mfma" else torch.float32
    gdt = torch.bfloat16 if path == "mfma" else torch.float32
    oh, ow = out_size(in_h, in_w, up, padding)
    if tier == "mask":
        x = block_sign_input(n, in_h, in_w, c, c_p, seed, xdt, *MASK_INPUT[up])
    else:
        x = gauss(n, in_h, in_w, c, c_p, seed, xdt, 3.0)
    gout = gauss(n, oh, ow, c, c_p, seed + 1, gdt, gscale)
    os_, b = scale_bias(n, c, c_p, seed + 2)
    return x, gout, os_, b


# the chained-strip cases of the MFMA path: (padding, in_h, in_w); one sample of 16 channels, replicated by the test
CHAINED = {2: ([9, 8, 9, 8], 33, 245), 4: ([-6, -9, -6, -9], 33, 125)}
CHAINED_C = 16


def chained_inputs(up, tier):
    """(x, gout, oscale, bias) of one sample and one 16-channel block of a chained-strip case (f16 x, bf16 gout)."""
    pad, h, w = CHAINED[up]
    c = CHAINED_C
    oh, ow = out_size(h, w, up, pad)
    if tier == "mask":
        x = block_sign_input(1, h, w, c, c, 5 + up, torch.float16, *MASK_INPUT[up])
    else:
        x = gauss(1, h, w, c, c, 5 + up, torch.float16, 3.0)
    gout = gauss(1, oh, ow, c, c, 6 + up, torch.bfloat16)
    os_, b = scale_bias(1, c, c, 77 + up)
    return x, gout, os_, b


# ------------------------------------------------------------------ the reference
def _nchw(t, c):
    return t.double()[..., :c].permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _adjoint(fn, shape, cot):
    """J^T cot of the linear map fn at inputs of `shape` (autograd)."""
    z = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    fn(z).backward(cot)
    return z.grad


def reference(x, gout, fu, fd, up, padding, gain=GAIN, slope=0.2, clamp=256.0, flip=False, oscale=None, bias=None,
              eps_x=2.0 ** -11, kappa=KAPPA, c=None):
    """x [n, h, w, c_p], gout [n, oh, ow, c_p] as stored (any dtype); fu / fd taps; clamp < 0: none.  Returns a dict of
    NHWC fp64 tensors over the first `c` channels: ref, ref0 (unscaled), B, B0, A, A0, and ydot [n, c]."""
    c = x.shape[-1] if c is None else c
    n = x.shape[0]
    fu, fd = fu.double(), fd.double()
    cl = None if clamp < 0 else float(clamp)
    xr = _nchw(x, c).requires_grad_(True)
    go = _nchw(gout, c)
    kw = dict(up=up, down=2, padding=padding, flip_filter=bool(flip))
    sg3.filtered_lrelu(xr, fu, fd, None, gain=gain, slope=slope, clamp=cl, **kw).backward(go)
    ref0 = xr.grad
    os_ = torch.ones(n, c, dtype=torch.float64) if oscale is None else oscale.double()[:, :c]
    bi = torch.zeros(c, dtype=torch.float64) if bias is None else bias.double()[:c]
    osb = os_[:, :, None, None]
    xd = xr.detach()
    ydot = (ref0 * (xd - bi[None, :, None, None])).sum(dim=(2, 3))
    # B: |taps|, |gout|, slope 1, no clamp
    B0 = _adjoint(lambda z: sg3.filtered_lrelu(z, fu.abs(), fd.abs(), None, gain=gain, slope=1.0, clamp=None, **kw),
                  xd.shape, go.abs())
    # A: fragile grid positions
    up_kw = dict(up=up, padding=padding, gain=up ** 2, flip_filter=bool(flip))
    U = sg3.upfirdn2d(xd, fu, **up_kw)
    Ua = sg3.upfirdn2d(xd.abs(), fu.abs(), **up_kw)
    dU = kappa * eps_x * Ua
    gD = _adjoint(lambda v: sg3.upfirdn2d(v, fd.abs(), down=2, flip_filter=bool(flip)), U.shape, go.abs())
    w = torch.zeros_like(U)
    if slope != 1.0:
        w = torch.where(U.abs() < dU, torch.full_like(U, 1.0 - slope), w)
    if cl is not None:
        br = torch.where(U > 0, torch.ones_like(U), torch.full_like(U, slope))   # slope of the lrelu branch
        near = ((U * br).abs() * gain - cl).abs() < dU * br * gain
        w = torch.where(near, torch.maximum(w, br), w)
    A0 = _adjoint(lambda z: sg3.upfirdn2d(z, fu.abs(), **up_kw), xd.shape, w * gain * gD)
    return dict(ref=_nhwc(ref0 * osb), ref0=_nhwc(ref0), B=_nhwc(B0 * osb.abs()), B0=_nhwc(B0),
                A=_nhwc(A0 * osb.abs()), A0=_nhwc(A0), ydot=ydot, fragile=(w > 0).double().mean().item(),
                x=_nhwc(xd), os=os_, bias=bi)


# ------------------------------------------------------------------ brute force (pins sg3's conventions)
def upfirdn_bruteforce(x, f, up, down, padding, flip, gain=1.0):
    """One plane [h, w] -> the definition as loops: zero-insert, pad or crop, correlate with the flipped filter
    (unflipped when `flip`), keep every down-th sample.  f is 1-D (separable)."""
    px0, px1, py0, py1 = padding
    h, w = x.shape
    z = [[0.0] * (w * up) for _ in range(h * up)]
    for i in range(h):
        for j in range(w):
            z[i * up][j * up] = float(x[i, j])

    def at(yy, xx):   # padded / cropped image, origin moved by the leading padding
        yy, xx = yy - py0, xx - px0
        return z[yy][xx] if 0 <= yy < h * up and 0 <= xx < w * up else 0.0

    ph, pw = h * up + py0 + py1, w * up + px0 + px1
    t = len(f)
    k = [float(v) * math.sqrt(gain) for v in f]   # gain ** (ndim / 2) per 1-D pass
    if not flip:
        k = k[::-1]
    oh, ow = ph - t + 1, pw - t + 1
    out = torch.zeros((oh + down - 1) // down, (ow + down - 1) // down, dtype=torch.float64)
    for oy in range(0, oh, down):
        for ox in range(0, ow, down):
            s = 0.0
            for a in range(t):
                for b in range(t):
                    s += k[a] * k[b] * at(oy + a, ox + b)
            out[oy // down, ox // down] = s
    return out


def flrelu_bruteforce(x, fu, fd, up, padding, gain, slope, clamp, flip):
    u = upfirdn_bruteforce(x, fu, up, 1, padding, flip, gain=up ** 2)
    v = torch.where(u > 0, u, u * slope) * gain
    if clamp >= 0:
        v = v.clamp(-clamp, clamp)
    return upfirdn_bruteforce(v, fd, 1, 2, [0, 0, 0, 0], flip)
