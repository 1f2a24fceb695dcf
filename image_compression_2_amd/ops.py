"""Where Python meets the C ABI (include/ic2ops.h): one keyword function per native launch family.

Each function takes tensors and named parameters, derives pointers, dtype codes and the stream, allocates the
workspaces the library asks for and launches through ``_native.call`` (looked up on the module at call time: the
benchmark's instrumented pass replaces it).  Before any launch it checks what the library cannot see: that every
tensor is contiguous, on the launch's device, of the dtype its code says, and at least as large as the geometry
implies -- the conditions under which the C side would read or write outside a buffer.  The checks compare Python
ints only (no sync, no allocation).  The modules above (stylegan3_hvae_full, networks_stylegan3, autograd_ops) call
these and never spell the ABI themselves.

Two assumptions: the launch's device is the first tensor's, so a CPU tensor there is refused only when
``_native.stream_of`` asks for its stream (the public entry points refuse it earlier, ``_native.require_gpu``); and
the forward ``flrelu`` takes one size per side, the synthesis activations being square.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nv

_DT = {nv.F32: torch.float32, nv.BF16: torch.bfloat16, nv.F16: torch.float16, nv.BF16X3: torch.bfloat16,
       nv.F16X2: torch.float16, nv.F16_IEEE: torch.float16}
_F32 = torch.float32


def _p(fn, what, t, dev, need, dt=_F32, opt=False):
    """Checked device pointer (an int: ctypes passes it as void*) of tensor `t` for entry point `fn`: on `dev`,
    contiguous, of torch dtype `dt` (None: any), at least `need` elements.  opt: None passes as a null pointer."""
    if t is None:
        if opt:
            return None
        raise ValueError(f"{fn}: {what} is required")
    if t.device != dev or not t.is_contiguous() or t.numel() < need or (dt is not None and t.dtype is not dt):
        if t.device != dev:
            raise ValueError(f"{fn}: {what} is on {t.device}, the launch on {dev}")
        if not t.is_contiguous():
            raise ValueError(f"{fn}: {what} is not contiguous")
        if t.numel() < need:
            raise ValueError(f"{fn}: {what} has {t.numel()} elements, the geometry needs {need}")
        raise TypeError(f"{fn}: {what} is {t.dtype}, the call says {dt}")
    return t.data_ptr()


def _dp(t):
    """Pointer (an int, as _p returns) of a tensor the wrapper allocated itself, or None.  nv.ptr builds a c_void_p per
    call; with it, and with conv's three small helper calls below not inlined, the alternated benchmark fell below
    the parent's spread at batch 1 (profiles/r22_ops_layer.txt, section 3), so the hot path keeps the cheap spelling."""
    return None if t is None else t.data_ptr()


def _taps(fn, what, f, ndim=1, opt=False):
    """(host pointer, taps) of a FIR filter held as a float32 numpy array (the kernels take taps from host memory)."""
    if f is None:
        if opt:
            return None, 1
        raise ValueError(f"{fn}: {what} is required")
    if f.dtype != np.float32 or not f.flags.c_contiguous or f.ndim != ndim or (ndim == 2 and f.shape[0] != f.shape[1]):
        raise TypeError(f"{fn}: {what} must be a contiguous float32 array of {ndim} equal dimension(s), got "
                        f"{f.dtype} {f.shape}")
    return f.ctypes.data_as(ctypes.c_void_p), f.shape[0]


def _kk(k):
    return (k, k) if isinstance(k, int) else k


def _act_width(code, cin_p):
    """Stored channels per pixel of a conv operand whose GEMM K is cin_p (the split layouts store [hi | lo] / x)."""
    return cin_p * 2 // 3 if code == nv.BF16X3 else cin_p // 2 if code == nv.F16X2 else cin_p


def _empty(shape, dt, dev):
    return torch.empty(shape, dtype=dt, device=dev)


# ------------------------------------------------------------------------------------------------ conv
def conv(x, w, y, code, n, h, w_, cin_p, cout_p, cout_valid, k, pad, *, oscale=None, bias=None, act=nv.ACT_LINEAR,
         in_layout=nv.NHWC, slope=0.0, gain=1.0, clamp=-1.0, out_mul=1.0, out_layout=nv.NHWC, out_code=None,
         flops=None, wino=None):
    """y = act((conv(x, w) * oscale[n][o] + bias[o]) * gain, clamp) * out_mul: ic2_conv_igemm_ws (with its split-K
    workspace), or ic2_conv_wino where `wino` (a callable returning the Winograd pack U) is given and the library's
    plan prefers it.  code: the operand code (IC2_BF16X3 / IC2_F16X2: cin_p is the GEMM K, x stores [hi | lo] / x);
    k: int or (kh, kw); out_code: y's dtype code (default: from y.dtype; IC2_F16_IEEE for gradients).  flops: the
    algorithmic FLOPs announced for this launch (nv.note_flops)."""
    kh, kw = (k, k) if k.__class__ is int else k   # _kk, inlined (see _dp)
    ho, wo = h + 2 * pad - kh + 1, w_ + 2 * pad - kw + 1
    dt = _DT[code]
    if out_code is None:
        out_code, ydt = nv.dtype_code(y.dtype), None
    else:
        ydt = _DT[out_code]
    if flops is not None:
        nv.note_flops(flops)
    use_wino = wino is not None and nv.wino_preferred(code, n, h, w_, cin_p, cout_p, kh, kw, pad)
    fn = "ic2_conv_wino" if use_wino else "ic2_conv_igemm_ws"
    dev = x.device
    px = _p(fn, "x", x, dev, n * h * w_ * (cin_p if code < nv.BF16X3 else _act_width(code, cin_p)), dt)
    py = _p(fn, "y", y, dev, n * ho * wo * (cout_valid if out_layout == nv.NCHW else cout_p), ydt)
    po = None if oscale is None else _p(fn, "oscale", oscale, dev, n * cout_p)
    pb = None if bias is None else _p(fn, "bias", bias, dev, cout_p)
    a = act | (in_layout << 4)   # nv.act_in_layout, inlined
    if use_wino:
        pu = _p(fn, "u", wino(), dev, cout_p * 12 * cin_p, torch.float16)
        nv.conv_wino(px, pu, py, code, out_code, n, h, w_, cin_p, cout_p, cout_valid, pad, ho, wo, po, pb, a, slope,
                     gain, clamp, out_mul, out_layout, nv.stream_of(x))
    else:
        pw = _p(fn, "w", w, dev, cout_p * kh * kw * cin_p, dt)
        nv.conv_igemm(px, pw, py, code, out_code, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, ho, wo, po, pb, a,
                      slope, gain, clamp, out_mul, out_layout, nv.stream_of(x), dev)
    return y


def conv_gn_fuses(code, n, h, w_, cin_p, cout_p, cout_valid, k, pad, groups, fuse=-1):
    """True when conv_gn with these arguments takes the GroupNorm statistics from the conv's epilogue."""
    kh, kw = _kk(k)
    return bool(nv.query("ic2_conv3x3_gn_fuses", code, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, groups,
                         int(fuse)))


def conv_gn(x, w, y, code, n, h, w_, cin_p, cout_p, cout_valid, k, pad, bias, groups, eps, *, out_mul=1.0, fuse=-1,
            flops=None):
    """y = conv(x, w) + bias and the GroupNorm (mean, rstd) of y -> the stats buffer (ic2_conv3x3_gn_fwd; for
    IC2_F16X2 operands ic2_conv3x3_gn_fwd_scaled, y = (conv + bias) * out_mul).  The plain codes get the conv's
    split-K workspace; the split ones run the halo GEMM, which has none."""
    kh, kw = _kk(k)
    fn = "ic2_conv3x3_gn_fwd_scaled" if code == nv.F16X2 else "ic2_conv3x3_gn_fwd"
    dev = x.device
    px = _p(fn, "x", x, dev, n * h * w_ * _act_width(code, cin_p), _DT[code])
    pw = _p(fn, "w", w, dev, cout_p * kh * kw * cin_p, _DT[code])
    ydt = torch.float32 if code == nv.BF16X3 else _DT[code]
    py = _p(fn, "y", y, dev, n * (h + 2 * pad - kh + 1) * (w_ + 2 * pad - kw + 1) * cout_p, ydt)
    pb = _p(fn, "bias", bias, dev, cout_p)
    nfl = int(nv.query("ic2_conv3x3_gn_stats_floats", code, n, h, w_, cin_p, cout_p, kh, kw, pad, groups))
    stats = _empty([nfl], _F32, dev)
    ws, nbytes = None, 0
    if code not in (nv.BF16X3, nv.F16X2):
        nbytes = int(nv.query("ic2_conv_igemm_ws_bytes", code, n, h, w_, cin_p, cout_p, kh, kw, pad))
        ws = _empty([max(nbytes, 16) // 4], _F32, dev) if nbytes > 0 else None
    if flops is not None:
        nv.note_flops(flops)
    mul = (float(out_mul),) if code == nv.F16X2 else ()
    nv.call(fn, px, pw, py, code, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, pb, *mul, groups, float(eps),
            _dp(stats), nfl, _dp(ws), nbytes, int(fuse), nv.stream_of(x))
    return stats


def from_rgb_conv(variant, x, w, bias, y, n, h, w_, cin, wdim, cout_p, *, flops=None):
    """The direct from_rgb conv on the NCHW f32 image.  variant "": bf16 weights packed [cout_p][3][3][wdim = cin_p],
    y bf16 (ic2_from_rgb_conv); "x3" / "f16": raw f32 weights [wdim = cout][cin][3][3], exact f32 arithmetic, y stored
    split bf16 [hi | lo] / rounded once to f16 (ic2_from_rgb_conv_x3 / _f16)."""
    fn = {"": "ic2_from_rgb_conv", "x3": "ic2_from_rgb_conv_x3", "f16": "ic2_from_rgb_conv_f16"}[variant]
    dev = x.device
    px = _p(fn, "x", x, dev, n * cin * h * w_)
    if variant == "":
        pw = _p(fn, "w", w, dev, cout_p * 9 * wdim, torch.bfloat16)
    else:
        pw = _p(fn, "w", w, dev, wdim * cin * 9)
    pb = _p(fn, "bias", bias, dev, cout_p)
    py = _p(fn, "y", y, dev, n * h * w_ * cout_p * (2 if variant == "x3" else 1),
            torch.float16 if variant == "f16" else torch.bfloat16)
    if flops is not None:
        nv.note_flops(flops)
    nv.call(fn, px, cin, pw, wdim, pb, py, n, h, w_, cout_p, nv.stream_of(x))
    return y


def wgrad_oihw(x, dy, n, h, w_, cin_p, cout_p, cout, cin, k, pad):
    """nn.Conv2d's weight gradient dw [cout][cin][kh][kw] f32 from x and dy NHWC (ic2_conv_wgrad_oihw + workspace)."""
    kh, kw = _kk(k)
    fn, dev, code = "ic2_conv_wgrad_oihw", x.device, nv.dtype_code(x.dtype)
    px = _p(fn, "x", x, dev, n * h * w_ * cin_p, None)
    pdy = _p(fn, "dy", dy, dev, n * (h + 2 * pad - kh + 1) * (w_ + 2 * pad - kw + 1) * cout_p, x.dtype)
    nfl = int(nv.query("ic2_conv_wgrad_ws_floats", n, h, w_, cin_p, cout_p, kh, kw, pad))
    ws = _empty([max(nfl, 4)], _F32, dev)
    dw = _empty([cout, cin, kh, kw], _F32, dev)   # the parameter's layout
    nv.call(fn, px, pdy, _dp(dw), code, n, h, w_, cin_p, cout_p, cout, cin, kh, kw, pad, _dp(ws), nfl,
            nv.stream_of(x))
    return dw


# ------------------------------------------------------------------------------------------------ weight packing
def _f32_weight(w):
    return w.detach().to(_F32).contiguous()


def pack_weight(w, cout_p, cin_p, dt, *, code=None, prenorm=0, scale=1.0, wsq=False):
    """w [cout][cin][kh][kw] (or [cout][cin], a 1x1) f32 -> packed [cout_p][kh][kw][cin_p] dt times scale
    (ic2_pack_weight); code IC2_BF16X3 / IC2_F16X2: the last dimension tripled [hi | lo | hi] / doubled [hi | lo].
    wsq: also return sum_k w_norm^2 [cout][cin] f32 (with prenorm)."""
    fn = "ic2_pack_weight"
    w = _f32_weight(w)
    cout, cin = w.shape[:2]
    kh, kw = (1, 1) if w.ndim == 2 else w.shape[2:]
    code = nv.dtype_code(dt) if code is None else code
    kp = cin_p * (3 if code == nv.BF16X3 else 2 if code == nv.F16X2 else 1)
    if cout > cout_p or cin > cin_p:
        raise ValueError(f"{fn}: weight {tuple(w.shape)} exceeds the padded [{cout_p}, {cin_p}]")
    out = _empty([cout_p, kp] if w.ndim == 2 else [cout_p, kh, kw, kp], dt, w.device)
    sq = _empty([cout, cin], _F32, w.device) if wsq else None
    nv.call(fn, _dp(w), cout, cin, kh, kw, cout_p, cin_p, int(prenorm), float(scale), _p(fn, "w_out", out, w.device, 0,
            _DT[code]), code, _dp(sq), nv.stream_of(w))
    return (out, sq) if wsq else out


def pack_weight_adjoint(w, cin_p, cout_p, dt):
    """w [cout][cin][kh][kw] f32 -> the dgrad pack [cin_p][kh][kw][cout_p] dt: flipped in space, transposed in
    channels (ic2_pack_weight_adjoint)."""
    fn = "ic2_pack_weight_adjoint"
    w = _f32_weight(w)
    cout, cin, kh, kw = w.shape
    if cout > cout_p or cin > cin_p:
        raise ValueError(f"{fn}: weight {tuple(w.shape)} exceeds the padded [{cout_p}, {cin_p}]")
    out = _empty([cin_p, kh, kw, cout_p], dt, w.device)
    nv.call(fn, _dp(w), cout, cin, kh, kw, cin_p, cout_p, _dp(out), nv.dtype_code(dt), nv.stream_of(w))
    return out


def pack_weight_wino(w, cout_p, cin_p, *, prenorm=0, scale=1.0):
    """w [cout][cin][3][3] f32 -> the Winograd F(2,3)-along-x pack U [cout_p][3][4][cin_p] f16 (ic2_pack_weight_wino)."""
    fn = "ic2_pack_weight_wino"
    w = _f32_weight(w)
    cout, cin, kh, kw = w.shape
    if (kh, kw) != (3, 3) or cout > cout_p or cin > cin_p:
        raise ValueError(f"{fn}: weight {tuple(w.shape)} is not a 3x3 within the padded [{cout_p}, {cin_p}]")
    u = _empty([cout_p, 3, 4, cin_p], torch.float16, w.device)
    nv.call(fn, _dp(w), cout, cin, cout_p, cin_p, int(prenorm), float(scale), _dp(u), nv.F16, nv.stream_of(w))
    return u


# ------------------------------------------------------------------------------------------------ filtered lrelu
def flrelu(x, y, n, c_p, in_size, out_size, fu, fd, up, down, padding, gain, slope, clamp, *, post_scale=None,
           blocked=False, out_blocked=False, radial=None):
    """The fused filtered lrelu on the conv output x NHWC [n, in, in, c_p] (blocked: [n, c_p/16, in, in, 16]) -> y
    [n, out, out, c_p] (out_blocked: channel-blocked too), times post_scale [n][c_p].  fu / fd: host float32 taps
    (None: one tap).  radial: None for a separable fd, else (rank, fd_v, fd_h) with fd [taps][taps] (the _2d entries).
    Entry: ic2_flrelu_nhwc(16)(_2d) from blocked / radial."""
    fn = ("ic2_flrelu_nhwc16" if blocked else "ic2_flrelu_nhwc") + ("" if radial is None else "_2d")
    dev = x.device
    px = _p(fn, "x", x, dev, n * in_size * in_size * c_p, None)
    py = _p(fn, "y", y, dev, n * out_size * out_size * c_p, None)
    pp = _p(fn, "post_scale", post_scale, dev, n * c_p, opt=True)
    pfu, nfu = _taps(fn, "fu", fu, opt=True)
    px0, px1, py0, py1 = padding
    out_code = nv.dtype_code(y.dtype) | (nv.flr_out_layout(nv.NHWC16) if out_blocked else 0)
    if radial is None:
        pfd, nfd = _taps(fn, "fd", fd, opt=True)
        mid = (None,)
    else:
        pfd, nfd = _taps(fn, "fd", fd, ndim=2)
        rank, fdv, fdh = radial
        for what, f in (("fd_v", fdv), ("fd_h", fdh)):
            if rank and (f is None or f.dtype != np.float32 or not f.flags.c_contiguous or f.shape != (rank, nfd)):
                raise TypeError(f"{fn}: {what} must be a contiguous float32 [{rank}, {nfd}] array")
        hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        mid = (rank, hp(fdv), hp(fdh), None)
    nv.call(fn, px, py, nv.dtype_code(x.dtype), out_code, n, c_p, in_size, in_size, out_size, out_size, pfu, nfu, pfd,
            nfd, *mid, up, down, px0, px1, py0, py1, float(gain), float(slope), float(clamp), 0, pp, nv.stream_of(x))
    return y


def flrelu_bwd(x, gout, gx, n, c_p, in_h, in_w, fu, fd, up, down, padding, gain, slope, clamp, *, radial=False,
               store=False, mul=None, bias=None):
    """Backward of flrelu w.r.t. its input: x the forward's input NHWC [n, in_h, in_w, c_p], gout the output gradient
    [n, oh, ow, c_p] -> gx.  store=False: the plain entry (ic2_flrelu_bwd_nhwc, gx f32; radial: ic2_flrelu_bwd_nhwc_2d
    without its store options).  store=True: the modulated conv's backward fused into the store (ic2_flrelu_bwd_nhwc_ex,
    radial: _2d): gx = dL/dx * mul[n][c] in gx's dtype, and the ydot partials of dL/dx * (x - bias[c]).
    -> (a fused instance ran, ydot or None); not run (IC2_E_UNSUPPORTED): nothing written, the caller composes."""
    fn = "ic2_flrelu_bwd_nhwc_2d" if radial else "ic2_flrelu_bwd_nhwc_ex" if store else "ic2_flrelu_bwd_nhwc"
    dev = x.device
    oh, ow = gout.shape[1], gout.shape[2]
    px = _p(fn, "x", x, dev, n * in_h * in_w * c_p, None)
    pg = _p(fn, "gout", gout, dev, n * oh * ow * c_p, None)
    pgx = _p(fn, "gx", gx, dev, n * in_h * in_w * c_p, None if radial or store else _F32)
    pfu, nfu = _taps(fn, "fu", fu)
    pfd, nfd = _taps(fn, "fd", fd, ndim=2 if radial else 1)
    px0, px1, py0, py1 = padding
    ydot, tail = None, ()
    if radial or store:
        pm = _p(fn, "mul", mul, dev, n * c_p, opt=True)
        pb = _p(fn, "bias", bias, dev, c_p, opt=True)
        nyd = 0
        if store:
            nyd = int(nv.query("ic2_flrelu_bwd_2d_ydot_floats" if radial else "ic2_flrelu_bwd_ydot_floats", n, c_p,
                               in_h, in_w, up))
            ydot = _empty([nyd], _F32, dev)
        tail = (pm, pb, _dp(ydot), nyd)
    gxc = (nv.dtype_code(gx.dtype),) if radial or store else ()
    ran = nv.try_call(fn, px, nv.dtype_code(x.dtype), pg, nv.dtype_code(gout.dtype), pgx, *gxc, n, c_p, in_h,
                      in_w, oh, ow, pfu, nfu, pfd, nfd, up, down, px0, px1, py0, py1, float(gain), float(slope),
                      float(clamp), 0, *tail, nv.stream_of(x))
    return ran, ydot


# ------------------------------------------------------------------------------------------------ GroupNorm, pooling
def gn_stats(y, n, hw, c_p, c, groups, eps):
    """GroupNorm (mean, rstd) of y NHWC by the two-stage pass (ic2_group_norm_stats) -> the stats buffer."""
    fn = "ic2_group_norm_stats"
    py = _p(fn, "y", y, y.device, n * hw * c_p, None)
    nfl = int(nv.query("ic2_group_norm_stats_floats", n, hw, groups))
    stats = _empty([nfl], _F32, y.device)
    nv.call(fn, py, nv.dtype_code(y.dtype), n, hw, c_p, c, groups, float(eps), _dp(stats), nv.stream_of(y))
    return stats


def gn_lrelu_pool(y, out, out_code, n, h, w_, c_p, c, groups, stats, gamma, beta, slope, pool):
    """GroupNorm apply -> leaky_relu (-> 2x2 average pool) (ic2_gn_lrelu_pool); out_code IC2_BF16X3: out stored split
    [hi | lo], 2 * c_p wide."""
    fn, dev = "ic2_gn_lrelu_pool", y.device
    oh, ow = (h // 2, w_ // 2) if pool else (h, w_)
    py = _p(fn, "y", y, dev, n * h * w_ * c_p, None)
    po = _p(fn, "out", out, dev, n * oh * ow * c_p * (2 if out_code == nv.BF16X3 else 1), _DT[out_code])
    ps = _p(fn, "stats", stats, dev, 2 * n * groups)
    nv.call(fn, py, po, nv.dtype_code(y.dtype), out_code, n, h, w_, c_p, c, groups, ps, _p(fn, "gamma", gamma, dev, c),
            _p(fn, "beta", beta, dev, c), float(slope), int(pool), nv.stream_of(y))
    return out


def gn_lrelu_pool_bwd(y, dout, n, h, w_, c_p, c, groups, stats, gamma, beta, slope, pool):
    """Backward of gn_lrelu_pool (ic2_gn_lrelu_pool_bwd_db + workspace) -> (dy like y, dgamma, dbeta, dsum [c] f32);
    dsum = the sum of dy over (n, p), the producing conv's bias gradient."""
    fn, dev = "ic2_gn_lrelu_pool_bwd_db", y.device
    oh, ow = (h // 2, w_ // 2) if pool else (h, w_)
    py = _p(fn, "y", y, dev, n * h * w_ * c_p, None)
    pd = _p(fn, "dout", dout, dev, n * oh * ow * c_p, None)
    ps = _p(fn, "stats", stats, dev, 2 * n * groups)
    pg, pb = _p(fn, "gamma", gamma, dev, c), _p(fn, "beta", beta, dev, c)
    nfl = int(nv.query("ic2_gn_lrelu_pool_bwd_floats", n, h, w_, c_p, groups))
    ws = _empty([nfl], _F32, dev)
    dy = torch.empty_like(y)
    dgamma, dbeta, dsum = _empty([c], _F32, dev), _empty([c], _F32, dev), _empty([c], _F32, dev)
    nv.call(fn, py, pd, _dp(dy), nv.dtype_code(y.dtype), nv.dtype_code(dout.dtype), nv.dtype_code(dy.dtype), n, h,
            w_, c_p, c, groups, ps, pg, pb, float(slope), int(pool), _dp(dgamma), _dp(dbeta), _dp(dsum),
            _dp(ws), nfl, nv.stream_of(y))
    return dy, dgamma, dbeta, dsum


def gap(x, code, n, hw, c_p, c):
    """Global average pool of x NHWC (ic2_global_avg_pool) -> its f32 buffer; [: n * c] holds [n][c]."""
    fn = "ic2_global_avg_pool"
    px = _p(fn, "x", x, x.device, n * hw * c_p * (2 if code == nv.BF16X3 else 1), _DT[code])
    nfl = int(nv.query("ic2_global_avg_pool_floats", n, hw, c_p, c))
    buf = _empty([nfl], _F32, x.device)
    nv.call(fn, px, code, n, hw, c_p, c, _dp(buf), nv.stream_of(x))
    return buf


def gap_bwd(dp, shape, dt, c):
    """Backward of gap: dpooled [n][c] f32 -> dx of `shape` [n, h, w, c_p] and dtype dt (ic2_gap_bwd)."""
    fn = "ic2_gap_bwd"
    n, h, w_, c_p = shape
    pd = _p(fn, "dpooled", dp, dp.device, n * c)
    dx = _empty(shape, dt, dp.device)
    nv.call(fn, pd, _dp(dx), nv.dtype_code(dt), n, h * w_, c_p, c, nv.stream_of(dp))
    return dx


# ------------------------------------------------------------------------------------------------ modulation scaling
def scale(x, xs, n, hw, c_p):
    """a = x * xscale[n][c] on NHWC (ic2_scale_nhwc)."""
    fn, dev = "ic2_scale_nhwc", x.device
    px, ps = _p(fn, "x", x, dev, n * hw * c_p, None), _p(fn, "xscale", xs, dev, n * c_p)
    a = torch.empty_like(x)
    nv.call(fn, px, ps, _dp(a), nv.dtype_code(x.dtype), n, hw, c_p, nv.stream_of(x))
    return a


def scale_bwd(da, x, xs, n, hw, c_p, *, want_dx=True, div=False):
    """Backward of scale (ic2_scale_bwd_nhwc, then ic2_colsum_div over its partial sums) -> (dx = da * xscale, or None
    without want_dx; sum_p da * x [n][c_p] f32 -- div: divided by xscale, 0 where that is 0)."""
    fn, dev = "ic2_scale_bwd_nhwc", x.device
    pda = _p(fn, "da", da, dev, n * hw * c_p, x.dtype)
    px, ps = _p(fn, "x", x, dev, n * hw * c_p, None), _p(fn, "xscale", xs, dev, n * c_p)
    npart = int(nv.query("ic2_scale_bwd_part_floats", n, hw, c_p))
    part = _empty([npart], _F32, dev)
    dx = torch.empty_like(x) if want_dx else None
    nv.call(fn, pda, px, ps, _dp(dx), nv.dtype_code(x.dtype), n, hw, c_p, _dp(part), npart, nv.stream_of(x))
    return dx, nv.colsum_div(part, n, c_p, xs if div else None)


# ------------------------------------------------------------------------------------------------ layout
def to_nhwc(x, dt, c_p, *, scale=None, split=False):
    """NCHW f32 x -> NHWC [n, h, w, c_p] dt, zero padded, times scale [n][c_p] (ic2_nchw_to_nhwc); split: stored split
    bf16 [hi | lo], 2 * c_p wide (IC2_BF16X3)."""
    fn, dev = "ic2_nchw_to_nhwc", x.device
    n, c, h, w_ = x.shape
    px = _p(fn, "x", x, dev, 0)
    ps = _p(fn, "scale", scale, dev, n * c_p, opt=True)
    if c > c_p:
        raise ValueError(f"{fn}: {c} channels exceed the stride {c_p}")
    out = _empty([n, h, w_, 2 * c_p if split else c_p], dt, dev)
    nv.call(fn, px, _dp(out), nv.BF16X3 if split else nv.dtype_code(dt), n, c, h, w_, c_p, ps, nv.stream_of(x))
    return out


def to_nchw(x, n, c, h, w_, c_p):
    """NHWC x [n, h, w, c_p] -> NCHW f32 [n, c, h, w] (ic2_nhwc_to_nchw)."""
    fn = "ic2_nhwc_to_nchw"
    px = _p(fn, "x", x, x.device, n * h * w_ * c_p, None)
    if c > c_p:
        raise ValueError(f"{fn}: {c} channels exceed the stride {c_p}")
    y = _empty([n, c, h, w_], _F32, x.device)
    nv.call(fn, px, nv.dtype_code(x.dtype), _dp(y), n, c, h, w_, c_p, nv.stream_of(x))
    return y


# ------------------------------------------------------------------------------------------------ FC, modulation, input
def fc(x, ldx, weight, bias, n, in_f, out_f, *, w_gain=1.0, b_gain=1.0, act=nv.ACT_LINEAR, alpha=0.2, act_gain=1.0,
       out=None):
    """y [n][out_f] = act((x[n * ldx + i] . weight[o][i]) * w_gain + bias[o] * b_gain) * act_gain, f32 (ic2_fc)."""
    fn, dev = "ic2_fc", x.device
    px = _p(fn, "x", x, dev, (n - 1) * ldx + in_f if n > 0 else 0)
    pw = _p(fn, "weight", weight, dev, out_f * in_f)
    pb = _p(fn, "bias", bias, dev, out_f, opt=True)
    if out is None:
        out = _empty([n, out_f], _F32, dev)
    nv.call(fn, px, ldx, pw, pb, _p(fn, "out", out, dev, n * out_f), n, in_f, out_f, float(w_gain), float(b_gain), act,
            float(alpha), float(act_gain), nv.stream_of(x))
    return out


def modconv_prep(styles, wsq, n, cin, cout, cin_p, cout_p, demod, style_gain, input_gain, xs, os_):
    """The (de)modulation coefficients xscale [n][cin_p], oscale [n][cout_p] from styles [n][cin] (ic2_modconv_prep)."""
    fn, dev = "ic2_modconv_prep", styles.device
    nv.call(fn, _p(fn, "styles", styles, dev, n * cin), _p(fn, "wsq", wsq, dev, cout * cin), n, cin, cout, cin_p, cout_p,
            int(demod), float(style_gain), float(input_gain), _p(fn, "xscale_out", xs, dev, n * cin_p),
            _p(fn, "oscale_out", os_, dev, n * cout_p), None, nv.stream_of(styles))


def modconv_prep_batched(ws, ldx, n, w_dim, rec):
    """Every layer's affine FC + modconv_prep in three launches (ic2_modconv_prep_batched); rec: int64 [nl][16] host
    records (ic2ops.h; SynthesisLayer.mod_record)."""
    fn = "ic2_modconv_prep_batched"
    if rec.dtype != np.int64 or rec.ndim != 2 or rec.shape[1] != 16 or not rec.flags.c_contiguous:
        raise TypeError(f"{fn}: the layer records must be a contiguous int64 [nl, 16] array, got {rec.dtype} {rec.shape}")
    pw = _p(fn, "ws", ws, ws.device, (n - 1) * ldx + int(rec[:, 6].max()) + w_dim if n > 0 else 0)
    nv.call(fn, pw, ldx, n, w_dim, rec.shape[0], rec.ctypes.data_as(ctypes.c_void_p), nv.stream_of(ws))


def synth_input_features(t, freqs, phases, transform, n, c, c_p, size, sampling_rate, bandwidth, dt):
    """SynthesisInput's Fourier features NHWC [n, size, size, c_p] dt from the affine output t [n][4]
    (ic2_synth_input_features)."""
    fn, dev = "ic2_synth_input_features", t.device
    args = (_p(fn, "t", t, dev, n * 4), _p(fn, "freqs", freqs, dev, c * 2), _p(fn, "phases", phases, dev, c),
            _p(fn, "transform", transform, dev, 9))
    if c > c_p:
        raise ValueError(f"{fn}: {c} channels exceed the stride {c_p}")
    feats = _empty([n, size, size, c_p], dt, dev)
    nv.call(fn, *args, n, c, c_p, size, float(sampling_rate), float(bandwidth), _dp(feats), nv.dtype_code(dt),
            nv.stream_of(t))
    return feats


def reparameterize(p, eps, n, num_ws, w_dim, ws_total, off, w_out, m_out, lv_out):
    """(mean, logvar) = halves of p [n][num_ws][2 * w_dim], w = mean + eps * exp(logvar / 2) -> slots
    [off, off + num_ws) of the three [n][ws_total][w_dim] outputs (ic2_reparameterize)."""
    fn, dev = "ic2_reparameterize", p.device
    if off < 0 or off + num_ws > ws_total:
        raise ValueError(f"{fn}: slots [{off}, {off + num_ws}) exceed {ws_total}")
    outs = [_p(fn, what, t, dev, n * ws_total * w_dim) for what, t in (("w_out", w_out), ("mean_out", m_out),
                                                                        ("logvar_out", lv_out))]
    nv.call(fn, _p(fn, "params", p, dev, n * num_ws * w_dim * 2), _p(fn, "eps", eps, dev, n * num_ws * w_dim), n, num_ws,
            w_dim, ws_total, off, *outs, nv.stream_of(p))


# ------------------------------------------------------------------------------------------------ quantizers, resize
def quantize_uniform(w, bits, q, idx=None):
    """The compress() quantizer on f32 w -> q (and int32 indices idx), ic2_quantize_uniform."""
    fn, dev = "ic2_quantize_uniform", w.device
    nv.call(fn, _p(fn, "w", w, dev, 0), w.numel(), int(bits), _p(fn, "q_out", q, dev, w.numel()),
            _p(fn, "idx_out", idx, dev, w.numel(), torch.int32, opt=True), nv.stream_of(w))


def resize_bilinear(img, out, nc, h, w_, oh, ow):
    """F.interpolate(bilinear, align_corners=False) of nc f32 planes [h][w] -> [oh][ow] (ic2_resize_bilinear)."""
    fn, dev = "ic2_resize_bilinear", img.device
    nv.call(fn, _p(fn, "img", img, dev, nc * h * w_), _p(fn, "out", out, dev, nc * oh * ow), nc, h, w_, oh, ow,
            nv.stream_of(img))


def gumbel_quantize(z, codebook, logt, hard, seed, noise, disc, idx, psum):
    """The fused Gumbel-softmax quantizer with a device seed (ic2_gumbel_softmax_quantize_dseed): z [m] f32 against
    codebook [k] -> disc [m], idx [m] int64, psum [k] (the probabilities' column sums, accumulated)."""
    fn, dev = "ic2_gumbel_softmax_quantize_dseed", z.device
    m, k = z.numel(), codebook.numel()
    nv.call(fn, _p(fn, "z", z, dev, 0), m, _p(fn, "codebook", codebook, dev, 0), k, _p(fn, "log_tau", logt, dev, 1), 1.0,
            int(bool(hard)), _p(fn, "seed", seed, dev, 1, torch.int64, opt=True), 0,
            _p(fn, "noise", noise, dev, m * k, opt=True), _p(fn, "disc", disc, dev, m),
            _p(fn, "idx", idx, dev, m, torch.int64), _p(fn, "psum", psum, dev, k), nv.stream_of(z))


def gumbel_quantize_bwd(z, codebook, logt, seed, noise, g, q, want_dlogt):
    """Backward of gumbel_quantize (ic2_gumbel_softmax_quantize_bwd + workspace): g [m] the gradient of disc, q [k]
    the per-code gradient of the column sums (or None) -> (dz [m] f32, dlog_tau [1] f32 or None)."""
    fn, dev = "ic2_gumbel_softmax_quantize_bwd", z.device
    m, k = z.numel(), codebook.numel()
    args = (_p(fn, "z", z, dev, 0), m, _p(fn, "codebook", codebook, dev, 0), k, _p(fn, "log_tau", logt, dev, 1), 1.0,
            _p(fn, "seed", seed, dev, 1, torch.int64, opt=True), 0, _p(fn, "noise", noise, dev, m * k, opt=True),
            _p(fn, "g", g, dev, m), _p(fn, "q", q, dev, k, opt=True))
    dz = _empty(m, _F32, dev)
    dlogt = ws = None
    nbytes = 0
    if want_dlogt:
        nbytes = int(nv.query("ic2_gumbel_softmax_bwd_ws_bytes", m))
        ws = _empty([max(nbytes, 4) // 4], _F32, dev)
        dlogt = _empty(1, _F32, dev)
    nv.call(fn, *args, _dp(dz), _dp(dlogt), _dp(ws), nbytes, nv.stream_of(z))
    return dz, dlogt


# ------------------------------------------------------------------------------------------------ image I/O
def resample_u8(src, recs, tables, ws, out, n, c, oh, ow, max_rows, total_rows, *, lut=None):
    """Pillow's 8-bit resize of a ragged uint8 HWC batch in two launches (ic2_resample_u8): src the packed sources,
    recs [n][9] int64 device records, tables the int32 table blob, ws >= total_rows * ow * c bytes -> out uint8
    [n][oh][ow][c], or with lut [c][256] f32 out f32 [n][c][oh][ow] = lut[ch][value]."""
    fn, dev = "ic2_resample_u8", src.device
    u8 = torch.uint8
    nv.call(fn, _p(fn, "src", src, dev, 1, u8), _p(fn, "recs", recs, dev, 9 * n, torch.int64),
            _p(fn, "tables", tables, dev, 1, torch.int32), n, c, oh, ow, max_rows, total_rows,
            _p(fn, "ws", ws, dev, total_rows * ow * c, u8), ws.numel(),
            _p(fn, "out", out, dev, n * oh * ow * c, u8 if lut is None else _F32),
            _p(fn, "lut", lut, dev, c * 256, opt=True), nv.stream_of(src))
    return out


def image_to_u8(x, y, n, c, h, w_, mode):
    """f32 NCHW x [n][c][h][w] -> uint8 NHWC y [n][h][w][c] in one of the reference's three conversions
    (ic2_image_to_u8; mode nv.U8_EVAL / U8_SAVE_IMAGE / U8_REFERENCE)."""
    fn, dev = "ic2_image_to_u8", x.device
    need = n * c * h * w_
    nv.call(fn, _p(fn, "x", x, dev, need), _p(fn, "y", y, dev, need, torch.uint8), n, c, h, w_, int(mode),
            nv.stream_of(x))
    return y
