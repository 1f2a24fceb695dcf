"""CPU: image_compression_2_amd.ops, the keyword layer over the C ABI.  A fake library object stands in for libic2ops
(`nv._lib`) and records what reaches it: every wrapper's entry point and full positional tuple are compared with a
literal written from include/ic2ops.h (every scalar distinct, so two swapped ints cannot pass), and every size, dtype,
contiguity and device check raises before anything is recorded."""
import ctypes

import numpy as np
import pytest
import torch

from image_compression_2_amd import _native as nv
from image_compression_2_amd import ops

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
STREAM = 0xABC0
ANY = "any non-null pointer"   # a workspace / output the wrapper allocates itself


class FakeLib:
    def __init__(self, **ret):
        self.calls, self.ret = [], ret

    def ic2_last_error(self):
        return b"fake message"

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args)))
            return self.ret.get(name, 0)
        return fn


@pytest.fixture
def fake(monkeypatch):
    def install(**ret):
        lib = FakeLib(**ret)
        monkeypatch.setattr(nv, "_lib", lib)
        monkeypatch.setattr(nv, "stream_of", lambda t=None: ctypes.c_void_p(STREAM))
        monkeypatch.setattr(nv, "_flops_hook", lambda f: lib.calls.append(("note_flops", (f,))))
        return lib
    return install


def T(numel, dt=F32):
    return torch.zeros(int(numel), dtype=dt)


def P(t):
    """The address the library must receive for tensor / host array t (pointers are recorded as their integer value)."""
    return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def check(lib, names, entry, want):
    """The fake saw exactly `names` in order; the last one is `entry` with the positional tuple `want`."""
    assert [c[0] for c in lib.calls] == names
    name, got = lib.calls[-1]
    assert name == entry and len(got) == len(want), (name, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if w is ANY:
            assert type(g) is int and g > 4096, (i, g)
        else:
            assert g == w and type(g) is type(w), (i, g, w)


# ------------------------------------------------------------------ every wrapper: name and positional tuple
def test_conv_igemm(fake):
    lib = fake(ic2_conv_igemm_ws_bytes=64)
    x, w, y, os_, b = T(2 * 5 * 7 * 6, F16), T(8 * 3 * 2 * 6, F16), T(2 * 5 * 8 * 8), T(16), T(8)
    assert ops.conv(x, w, y, nv.F16, 2, 5, 7, 6, 8, 4, (3, 2), 1, oscale=os_, bias=b, act=nv.ACT_LRELU,
                    in_layout=nv.NHWC16, slope=0.25, gain=1.5, clamp=9.0, out_mul=0.5, out_layout=nv.NHWC16,
                    flops=12345) is y
    # x, w, y, dtype, out_dtype, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, ho, wo, oscale, bias, act, slope,
    # act_gain, clamp, out_mul, out_layout, ws, ws_bytes, stream
    check(lib, ["note_flops", "ic2_conv_igemm_ws_bytes", "ic2_conv_igemm_ws"], "ic2_conv_igemm_ws",
          (P(x), P(w), P(y), nv.F16, nv.F32, 2, 5, 7, 6, 8, 4, 3, 2, 1, 5, 8, P(os_), P(b), 1 | (2 << 4), 0.25, 1.5, 9.0,
           0.5, 2, ANY, 64, STREAM))
    assert lib.calls[1] == ("ic2_conv_igemm_ws_bytes", (nv.F16, 2, 5, 7, 6, 8, 3, 2, 1))


def test_conv_defaults_nchw_and_gradient_code(fake):
    lib = fake()
    x, w, y = T(2 * 5 * 7 * 6, F16), T(8 * 6, F16), T(2 * 5 * 7 * 4, F16)   # NCHW: cout_valid channels
    ops.conv(x, w, y, nv.F16, 2, 5, 7, 6, 8, 4, 1, 0, out_layout=nv.NCHW, out_code=nv.F16_IEEE)
    check(lib, ["ic2_conv_igemm_ws_bytes", "ic2_conv_igemm_ws"], "ic2_conv_igemm_ws",
          (P(x), P(w), P(y), nv.F16, nv.F16_IEEE, 2, 5, 7, 6, 8, 4, 1, 1, 0, 5, 7, None, None, 0, 0.0, 1.0, -1.0, 1.0, 1,
           None, 0, STREAM))


def test_conv_wino_rule(fake):
    lib = fake(ic2_conv_wino_preferred=1)
    x, u, y, os_, b = T(2 * 5 * 7 * 6, F16), T(8 * 12 * 6, F16), T(2 * 7 * 9 * 8, F16), T(16), T(8)
    packs = []
    ops.conv(x, None, y, nv.F16, 2, 5, 7, 6, 8, 4, 3, 2, oscale=os_, bias=b, in_layout=nv.NHWC16, out_layout=nv.NHWC16,
             wino=lambda: packs.append(1) or u, flops=77)
    # x, u, y, dtype, out_dtype, n, h, w_, cin_p, cout_p, cout_valid, pad, ho, wo, oscale, bias, act, slope, act_gain,
    # clamp, out_mul, out_layout, stream
    check(lib, ["note_flops", "ic2_conv_wino_preferred", "ic2_conv_wino"], "ic2_conv_wino",
          (P(x), P(u), P(y), nv.F16, nv.F16, 2, 5, 7, 6, 8, 4, 2, 7, 9, P(os_), P(b), 2 << 4, 0.0, 1.0, -1.0, 1.0, 2,
           STREAM))
    assert lib.calls[1] == ("ic2_conv_wino_preferred", (nv.F16, 2, 5, 7, 6, 8, 3, 3, 2)) and packs == [1]
    lib = fake(ic2_conv_wino_preferred=0)   # not preferred: the implicit GEMM, and the pack is never built
    w = T(8 * 9 * 6, F16)
    ops.conv(x, w, y, nv.F16, 2, 5, 7, 6, 8, 4, 3, 2, wino=lambda: 1 / 0)
    assert [c[0] for c in lib.calls] == ["ic2_conv_wino_preferred", "ic2_conv_igemm_ws_bytes", "ic2_conv_igemm_ws"]


def test_conv_gn(fake):
    lib = fake(ic2_conv3x3_gn_stats_floats=40, ic2_conv_igemm_ws_bytes=48, ic2_conv3x3_gn_fuses=1)
    assert ops.conv_gn_fuses(nv.BF16X3, 2, 5, 7, 9, 8, 4, (3, 6), 1, 16, fuse=0) is True
    assert lib.calls.pop() == ("ic2_conv3x3_gn_fuses", (nv.BF16X3, 2, 5, 7, 9, 8, 4, 3, 6, 1, 16, 0))
    x, w, y, b = T(2 * 5 * 7 * 6, BF16), T(8 * 3 * 9 * 6, BF16), T(2 * 5 * 1 * 8, BF16), T(8)   # k (3, 9): wo = 1
    stats = ops.conv_gn(x, w, y, nv.BF16, 2, 5, 7, 6, 8, 4, (3, 9), 1, b, 16, 1e-3, fuse=-1, flops=99)
    assert stats.shape == (40,) and stats.dtype == F32
    # x, w, y, dtype, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, bias, groups, eps, stats, stats_floats, conv_ws,
    # conv_ws_bytes, fuse, stream
    check(lib, ["ic2_conv3x3_gn_stats_floats", "ic2_conv_igemm_ws_bytes", "note_flops", "ic2_conv3x3_gn_fwd"],
          "ic2_conv3x3_gn_fwd", (P(x), P(w), P(y), nv.BF16, 2, 5, 7, 6, 8, 4, 3, 9, 1, P(b), 16, 1e-3, P(stats), 40, ANY,
                                 48, -1, STREAM))
    assert lib.calls[0][1] == (nv.BF16, 2, 5, 7, 6, 8, 3, 9, 1, 16) and lib.calls[1][1] == (nv.BF16, 2, 5, 7, 6, 8, 3, 9, 1)
    # split bf16: x stores [hi | lo] (2/3 of the GEMM K), y f32, no conv workspace
    lib = fake(ic2_conv3x3_gn_stats_floats=40)
    x, w, y = T(2 * 5 * 7 * 6, BF16), T(8 * 9 * 9, BF16), T(2 * 5 * 7 * 8, F32)
    stats = ops.conv_gn(x, w, y, nv.BF16X3, 2, 5, 7, 9, 8, 4, 3, 1, b, 16, 1e-3, fuse=1)
    check(lib, ["ic2_conv3x3_gn_stats_floats", "ic2_conv3x3_gn_fwd"], "ic2_conv3x3_gn_fwd",
          (P(x), P(w), P(y), nv.BF16X3, 2, 5, 7, 9, 8, 4, 3, 3, 1, P(b), 16, 1e-3, P(stats), 40, None, 0, 1, STREAM))
    # split-weight f16: the scaled entry, out_mul after bias
    lib = fake(ic2_conv3x3_gn_stats_floats=40)
    x, w, y = T(2 * 5 * 7 * 6, F16), T(8 * 9 * 12, F16), T(2 * 5 * 7 * 8, F16)
    stats = ops.conv_gn(x, w, y, nv.F16X2, 2, 5, 7, 12, 8, 4, 3, 1, b, 16, 1e-3, out_mul=0.125)
    check(lib, ["ic2_conv3x3_gn_stats_floats", "ic2_conv3x3_gn_fwd_scaled"], "ic2_conv3x3_gn_fwd_scaled",
          (P(x), P(w), P(y), nv.F16X2, 2, 5, 7, 12, 8, 4, 3, 3, 1, P(b), 0.125, 16, 1e-3, P(stats), 40, None, 0, -1,
           STREAM))


@pytest.mark.parametrize("variant,entry,wdt,ydt,ymul", [("", "ic2_from_rgb_conv", BF16, BF16, 1),
                                                        ("x3", "ic2_from_rgb_conv_x3", F32, BF16, 2),
                                                        ("f16", "ic2_from_rgb_conv_f16", F32, F16, 1)])
def test_from_rgb_conv(fake, variant, entry, wdt, ydt, ymul):
    lib = fake()
    wdim = 32 if variant == "" else 20
    x, b, y = T(2 * 3 * 5 * 7), T(64), T(2 * 5 * 7 * 64 * ymul, ydt)
    w = T(64 * 9 * 32, BF16) if variant == "" else T(20 * 3 * 9)
    ops.from_rgb_conv(variant, x, w, b, y, 2, 5, 7, 3, wdim, 64, flops=5)
    # x, cin, w, cin_p | cout, bias, y, n, h, w, cout_p, stream
    check(lib, ["note_flops", entry], entry, (P(x), 3, P(w), wdim, P(b), P(y), 2, 5, 7, 64, STREAM))


def test_wgrad_oihw(fake):
    lib = fake(ic2_conv_wgrad_ws_floats=24)
    # n, h, w, cin_p, cout_p, cout, cin, kh, kw, pad pairwise different: 9, 10, 7, 6, 8, 4, 3, 5, 2, 1
    x, dy = T(9 * 10 * 7 * 6, BF16), T(9 * 8 * 8 * 8, BF16)
    dw = ops.wgrad_oihw(x, dy, 9, 10, 7, 6, 8, 4, 3, (5, 2), 1)
    assert dw.shape == (4, 3, 5, 2) and dw.dtype == F32
    # x, dy, dw, dtype, n, h, w, cin_p, cout_p, cout, cin, kh, kw, pad, workspace, ws_floats, stream
    check(lib, ["ic2_conv_wgrad_ws_floats", "ic2_conv_wgrad_oihw"], "ic2_conv_wgrad_oihw",
          (P(x), P(dy), P(dw), nv.BF16, 9, 10, 7, 6, 8, 4, 3, 5, 2, 1, ANY, 24, STREAM))
    assert lib.calls[0][1] == (9, 10, 7, 6, 8, 5, 2, 1)


def test_pack_weight(fake):
    lib = fake()
    w = torch.zeros(4, 3, 5, 2)
    out, sq = ops.pack_weight(w, 8, 6, BF16, prenorm=True, scale=0.5, wsq=True)
    assert out.shape == (8, 5, 2, 6) and out.dtype == BF16 and sq.shape == (4, 3) and sq.dtype == F32
    # w, cout, cin, kh, kw, cout_p, cin_p, prenorm, scale, w_out, dtype, wsq_out, stream
    check(lib, ["ic2_pack_weight"], "ic2_pack_weight", (P(w), 4, 3, 5, 2, 8, 6, 1, 0.5, P(out), nv.BF16, P(sq), STREAM))
    for code, dt, mul in ((nv.BF16X3, BF16, 3), (nv.F16X2, F16, 2)):
        lib = fake()
        out = ops.pack_weight(w, 8, 6, dt, code=code)
        assert out.shape == (8, 5, 2, 6 * mul) and out.dtype == dt
        check(lib, ["ic2_pack_weight"], "ic2_pack_weight", (P(w), 4, 3, 5, 2, 8, 6, 0, 1.0, P(out), code, None, STREAM))
    lib = fake()
    w2 = torch.zeros(4, 3)   # SynthesisInput's 1x1 mix
    out = ops.pack_weight(w2, 8, 6, F32, scale=0.25)
    assert out.shape == (8, 6)
    check(lib, ["ic2_pack_weight"], "ic2_pack_weight", (P(w2), 4, 3, 1, 1, 8, 6, 0, 0.25, P(out), nv.F32, None, STREAM))
    with pytest.raises(ValueError, match="ic2_pack_weight"):
        ops.pack_weight(w, 3, 6, BF16)
    assert lib.calls[1:] == []


def test_pack_weight_adjoint_and_wino(fake):
    lib = fake()
    w = torch.zeros(4, 3, 5, 2)
    out = ops.pack_weight_adjoint(w, 6, 8, F16)
    assert out.shape == (6, 5, 2, 8) and out.dtype == F16
    # w, cout, cin, kh, kw, cin_p, cout_p, w_out, dtype, stream
    check(lib, ["ic2_pack_weight_adjoint"], "ic2_pack_weight_adjoint", (P(w), 4, 3, 5, 2, 6, 8, P(out), nv.F16, STREAM))
    lib = fake()
    w = torch.zeros(4, 5, 3, 3)
    u = ops.pack_weight_wino(w, 8, 6, prenorm=True, scale=0.5)
    assert u.shape == (8, 3, 4, 6) and u.dtype == F16
    # w, cout, cin, cout_p, cin_p, prenorm, scale, u_out, dtype, stream
    check(lib, ["ic2_pack_weight_wino"], "ic2_pack_weight_wino", (P(w), 4, 5, 8, 6, 1, 0.5, P(u), nv.F16, STREAM))
    for bad in (lambda: ops.pack_weight_wino(torch.zeros(4, 5, 1, 1), 8, 6), lambda: ops.pack_weight_wino(w, 8, 4),
                lambda: ops.pack_weight_adjoint(w, 4, 8, F16)):
        with pytest.raises(ValueError, match="ic2_pack_weight"):
            bad()
    assert len(lib.calls) == 1


FU = np.arange(12, dtype=np.float32)
FD = np.arange(8, dtype=np.float32)
FD2 = np.zeros([12, 12], np.float32)
FDV, FDH = np.zeros([3, 12], np.float32), np.ones([3, 12], np.float32)


@pytest.mark.parametrize("blocked,out_blocked", [(False, False), (True, True)])
def test_flrelu_separable(fake, blocked, out_blocked):
    lib = fake()
    x, y, ps = T(2 * 9 * 9 * 32, F16), T(2 * 11 * 11 * 32, BF16), T(64)
    ops.flrelu(x, y, 2, 32, 9, 11, FU, FD, 4, 3, [5, 6, 7, 8], 1.5, 0.25, 64.0, post_scale=ps, blocked=blocked,
               out_blocked=out_blocked)
    entry = "ic2_flrelu_nhwc16" if blocked else "ic2_flrelu_nhwc"
    # x, y, dtype_in, dtype_out, n, c_p, in_h, in_w, out_h, out_w, fu, fu_taps, fd, fd_taps, b, up, down, px0, px1, py0,
    # py1, gain, slope, clamp, flip, post_scale, stream
    check(lib, [entry], entry, (P(x), P(y), nv.F16, nv.BF16 | ((2 << 4) if out_blocked else 0), 2, 32, 9, 9, 11, 11, P(FU),
                                12, P(FD), 8, None, 4, 3, 5, 6, 7, 8, 1.5, 0.25, 64.0, 0, P(ps), STREAM))


def test_flrelu_defaults_and_radial(fake):
    lib = fake()
    x, y = T(2 * 9 * 9 * 32), T(2 * 11 * 11 * 32)
    ops.flrelu(x, y, 2, 32, 9, 11, None, None, 1, 1, [0, 0, 0, 0], 1.0, 0.2, -1.0)
    check(lib, ["ic2_flrelu_nhwc"], "ic2_flrelu_nhwc", (P(x), P(y), nv.F32, nv.F32, 2, 32, 9, 9, 11, 11, None, 1, None, 1,
                                                        None, 1, 1, 0, 0, 0, 0, 1.0, 0.2, -1.0, 0, None, STREAM))
    for blocked in (False, True):
        lib = fake()
        entry = "ic2_flrelu_nhwc16_2d" if blocked else "ic2_flrelu_nhwc_2d"
        ops.flrelu(x, y, 2, 32, 9, 11, FU, FD2, 4, 3, [5, 6, 7, 8], 1.5, 0.25, 64.0, blocked=blocked,
                   radial=(3, FDV, FDH))
        # ..., fd, fd_taps, rank, fd_v, fd_h, b, up, down, ...
        check(lib, [entry], entry, (P(x), P(y), nv.F32, nv.F32, 2, 32, 9, 9, 11, 11, P(FU), 12, P(FD2), 12, 3, P(FDV),
                                    P(FDH), None, 4, 3, 5, 6, 7, 8, 1.5, 0.25, 64.0, 0, None, STREAM))
    lib = fake()
    ops.flrelu(x, y, 2, 32, 9, 11, FU, FD2, 4, 3, [5, 6, 7, 8], 1.5, 0.25, 64.0, radial=(0, None, None))
    assert lib.calls[0][1][14:18] == (0, None, None, None)


def test_flrelu_bwd_entries(fake):
    x, g, ps, b = T(2 * 9 * 13 * 32, F16), T(2 * 10 * 11 * 32, BF16).view(2, 10, 11, 32), T(64), T(32)
    # the plain entry: x, x_dtype, gout, g_dtype, gx, n, c_p, in_h, in_w, out_h, out_w, fu, fu_taps, fd, fd_taps, up, down,
    # px0, px1, py0, py1, gain, slope, clamp, flip, stream
    lib = fake()
    gx = T(2 * 9 * 13 * 32)
    assert ops.flrelu_bwd(x, g, gx, 2, 32, 9, 13, FU, FD, 4, 3, [5, 6, 7, 8], 1.5, 0.25, 64.0) == (True, None)
    check(lib, ["ic2_flrelu_bwd_nhwc"], "ic2_flrelu_bwd_nhwc",
          (P(x), nv.F16, P(g), nv.BF16, P(gx), 2, 32, 9, 13, 10, 11, P(FU), 12, P(FD), 8, 4, 3, 5, 6, 7, 8, 1.5, 0.25, 64.0,
           0, STREAM))
    # radial without the store options: _2d with gx_dtype and null oscale / bias / ydot
    lib = fake()
    assert ops.flrelu_bwd(x, g, gx, 2, 32, 9, 13, FU, FD2, 4, 3, [5, 6, 7, 8], 1.5, 0.25, 64.0, radial=True) == (True, None)
    check(lib, ["ic2_flrelu_bwd_nhwc_2d"], "ic2_flrelu_bwd_nhwc_2d",
          (P(x), nv.F16, P(g), nv.BF16, P(gx), nv.F32, 2, 32, 9, 13, 10, 11, P(FU), 12, P(FD2), 12, 4, 3, 5, 6, 7, 8, 1.5,
           0.25, 64.0, 0, None, None, None, 0, STREAM))
    # the fused store: _ex / _2d, each with its own ydot query
    gxb = T(2 * 9 * 13 * 32, BF16)
    for radial, entry, query, fd in ((False, "ic2_flrelu_bwd_nhwc_ex", "ic2_flrelu_bwd_ydot_floats", FD),
                                     (True, "ic2_flrelu_bwd_nhwc_2d", "ic2_flrelu_bwd_2d_ydot_floats", FD2)):
        lib = fake(**{query: 56})
        ran, ydot = ops.flrelu_bwd(x, g, gxb, 2, 32, 9, 13, FU, fd, 4, 3, [5, 6, 7, 8], 1.5, 0.25, 64.0, radial=radial,
                                   store=True, mul=ps, bias=b)
        assert ran is True and ydot.shape == (56,) and ydot.dtype == F32
        # ..., flip, oscale, bias, ydot, ydot_floats, stream
        check(lib, [query, entry], entry,
              (P(x), nv.F16, P(g), nv.BF16, P(gxb), nv.BF16, 2, 32, 9, 13, 10, 11, P(FU), 12, P(fd), fd.shape[0], 4, 3, 5,
               6, 7, 8, 1.5, 0.25, 64.0, 0, P(ps), P(b), P(ydot), 56, STREAM))
        assert lib.calls[0][1] == (2, 32, 9, 13, 4)
    # no instance: not run, and reported so
    lib = fake(ic2_flrelu_bwd_nhwc=2)
    assert ops.flrelu_bwd(x, g, gx, 2, 32, 9, 13, FU, FD, 4, 3, [5, 6, 7, 8], 1.5, 0.25, 64.0)[0] is False
    lib = fake(ic2_flrelu_bwd_nhwc=1)
    with pytest.raises(RuntimeError, match="ic2_flrelu_bwd_nhwc failed .code 1.: fake message"):
        ops.flrelu_bwd(x, g, gx, 2, 32, 9, 13, FU, FD, 4, 3, [5, 6, 7, 8], 1.5, 0.25, 64.0)


def test_group_norm_wrappers(fake):
    lib = fake(ic2_group_norm_stats_floats=44)
    y = T(2 * 35 * 32, F16)
    stats = ops.gn_stats(y, 2, 35, 32, 30, 4, 1e-3)
    assert stats.shape == (44,)
    # y, dtype, n, hw, c_p, c, groups, eps, stats, stream
    check(lib, ["ic2_group_norm_stats_floats", "ic2_group_norm_stats"], "ic2_group_norm_stats",
          (P(y), nv.F16, 2, 35, 32, 30, 4, 1e-3, P(stats), STREAM))
    assert lib.calls[0][1] == (2, 35, 4)
    lib = fake()
    y, out, st, ga, be = T(2 * 6 * 8 * 32), T(2 * 3 * 4 * 32 * 2, BF16), T(2 * 2 * 4), T(30), T(30)
    ops.gn_lrelu_pool(y, out, nv.BF16X3, 2, 6, 8, 32, 30, 4, st, ga, be, 0.25, True)
    # y, out, dtype_in, dtype_out, n, h, w, c_p, c, groups, stats, gamma, beta, slope, pool, stream
    check(lib, ["ic2_gn_lrelu_pool"], "ic2_gn_lrelu_pool",
          (P(y), P(out), nv.F32, nv.BF16X3, 2, 6, 8, 32, 30, 4, P(st), P(ga), P(be), 0.25, 1, STREAM))
    lib = fake(ic2_gn_lrelu_pool_bwd_floats=52)
    yb, dout = T(2 * 6 * 8 * 32, BF16).view(2, 6, 8, 32), T(2 * 3 * 4 * 32, F16)
    dy, dg, db, ds = ops.gn_lrelu_pool_bwd(yb, dout, 2, 6, 8, 32, 30, 4, st, ga, be, 0.25, True)
    assert dy.shape == yb.shape and dy.dtype == BF16 and dg.shape == db.shape == ds.shape == (30,)
    # y, dout, dy, dtype_y, dtype_dout, dtype_dy, n, h, w, c_p, c, groups, stats, gamma, beta, slope, pool, dgamma, dbeta,
    # dsum, workspace, ws_floats, stream
    check(lib, ["ic2_gn_lrelu_pool_bwd_floats", "ic2_gn_lrelu_pool_bwd_db"], "ic2_gn_lrelu_pool_bwd_db",
          (P(yb), P(dout), P(dy), nv.BF16, nv.F16, nv.BF16, 2, 6, 8, 32, 30, 4, P(st), P(ga), P(be), 0.25, 1, P(dg), P(db),
           P(ds), ANY, 52, STREAM))
    assert lib.calls[0][1] == (2, 6, 8, 32, 4)


def test_gap_wrappers(fake):
    lib = fake(ic2_global_avg_pool_floats=72)
    x = T(2 * 35 * 32 * 2, BF16)
    buf = ops.gap(x, nv.BF16X3, 2, 35, 32, 30)
    assert buf.shape == (72,)
    # x, dtype, n, hw, c_p, c, out, stream
    check(lib, ["ic2_global_avg_pool_floats", "ic2_global_avg_pool"], "ic2_global_avg_pool",
          (P(x), nv.BF16X3, 2, 35, 32, 30, P(buf), STREAM))
    assert lib.calls[0][1] == (2, 35, 32, 30)
    lib = fake()
    dp = T(2 * 30)
    dx = ops.gap_bwd(dp, (2, 5, 7, 32), F16, 30)
    assert dx.shape == (2, 5, 7, 32) and dx.dtype == F16
    # dpooled, dx, dtype, n, hw, c_p, c, stream
    check(lib, ["ic2_gap_bwd"], "ic2_gap_bwd", (P(dp), P(dx), nv.F16, 2, 35, 32, 30, STREAM))


def test_scale_wrappers(fake):
    lib = fake()
    x, xs = T(2 * 35 * 32, BF16), T(64)
    a = ops.scale(x, xs, 2, 35, 32)
    # x, xscale, a, dtype, n, hw, c_p, stream
    check(lib, ["ic2_scale_nhwc"], "ic2_scale_nhwc", (P(x), P(xs), P(a), nv.BF16, 2, 35, 32, STREAM))
    lib = fake(ic2_scale_bwd_part_floats=128)
    da = T(2 * 35 * 32, BF16)
    dx, dxs = ops.scale_bwd(da, x, xs, 2, 35, 32)
    assert dx.shape == x.shape and dx.dtype == BF16 and dxs.shape == (2, 32)
    # da, x, xscale, dx, dtype, n, hw, c_p, part, part_floats, stream ; then part, n, rows, c, den, out, stream
    assert [c[0] for c in lib.calls] == ["ic2_scale_bwd_part_floats", "ic2_scale_bwd_nhwc", "ic2_colsum_div"]
    assert lib.calls[0][1] == (2, 35, 32)
    part = lib.calls[1][1][8]
    assert lib.calls[1][1] == (P(da), P(x), P(xs), P(dx), nv.BF16, 2, 35, 32, part, 128, STREAM) and part > 4096
    assert lib.calls[2][1] == (part, 2, 2, 32, None, P(dxs), STREAM)
    lib = fake(ic2_scale_bwd_part_floats=128)
    dx, dxs = ops.scale_bwd(da, x, xs, 2, 35, 32, want_dx=False, div=True)
    assert dx is None and lib.calls[1][1][3] is None and lib.calls[2][1][4] == P(xs)


def test_layout_wrappers(fake):
    lib = fake()
    x, sc = torch.zeros(2, 3, 5, 7), T(64)
    out = ops.to_nhwc(x, F16, 32, scale=sc)
    assert out.shape == (2, 5, 7, 32) and out.dtype == F16
    # x, y, dtype, n, c, h, w, c_p, scale, stream
    check(lib, ["ic2_nchw_to_nhwc"], "ic2_nchw_to_nhwc", (P(x), P(out), nv.F16, 2, 3, 5, 7, 32, P(sc), STREAM))
    lib = fake()
    out = ops.to_nhwc(x, BF16, 32, split=True)
    assert out.shape == (2, 5, 7, 64) and out.dtype == BF16
    check(lib, ["ic2_nchw_to_nhwc"], "ic2_nchw_to_nhwc", (P(x), P(out), nv.BF16X3, 2, 3, 5, 7, 32, None, STREAM))
    lib = fake()
    xn = T(2 * 5 * 7 * 32, BF16)
    y = ops.to_nchw(xn, 2, 3, 5, 7, 32)
    assert y.shape == (2, 3, 5, 7) and y.dtype == F32
    # x, dtype, y, n, c, h, w, c_p, stream
    check(lib, ["ic2_nhwc_to_nchw"], "ic2_nhwc_to_nchw", (P(xn), nv.BF16, P(y), 2, 3, 5, 7, 32, STREAM))
    for bad in (lambda: ops.to_nhwc(x, F16, 2), lambda: ops.to_nchw(xn, 2, 33, 5, 7, 32)):
        with pytest.raises(ValueError, match="ic2_n"):
            bad()
    assert len(lib.calls) == 1


def test_fc_and_modulation(fake):
    lib = fake()
    x, w, b = T(40 + 5), T(7 * 5), T(7)
    out = ops.fc(x, 40, w, b, 2, 5, 7, w_gain=0.5, b_gain=0.25, act=nv.ACT_LRELU, alpha=0.125, act_gain=1.5)
    assert out.shape == (2, 7)
    # x, ldx, w, b, y, n, in_f, out_f, w_gain, b_gain, act, alpha, act_gain, stream
    check(lib, ["ic2_fc"], "ic2_fc", (P(x), 40, P(w), P(b), P(out), 2, 5, 7, 0.5, 0.25, 1, 0.125, 1.5, STREAM))
    lib = fake()
    mine = T(14)
    assert ops.fc(x, 40, w, None, 2, 5, 7, out=mine) is mine
    check(lib, ["ic2_fc"], "ic2_fc", (P(x), 40, P(w), None, P(mine), 2, 5, 7, 1.0, 1.0, 0, 0.2, 1.0, STREAM))
    lib = fake()
    st, wsq, xs, os_ = T(2 * 5), T(7 * 5), T(2 * 32), T(2 * 64)
    ops.modconv_prep(st, wsq, 2, 5, 7, 32, 64, True, 0.5, 0.25, xs, os_)
    # styles, wsq, n, cin, cout, cin_p, cout_p, demod, style_gain, input_gain, xscale_out, oscale_out, scratch, stream
    check(lib, ["ic2_modconv_prep"], "ic2_modconv_prep",
          (P(st), P(wsq), 2, 5, 7, 32, 64, 1, 0.5, 0.25, P(xs), P(os_), None, STREAM))
    lib = fake()
    rec = np.zeros([3, 16], np.int64)
    rec[:, 6] = [10, 20, 30]
    ws = T(100 + 30 + 8)
    ops.modconv_prep_batched(ws, 100, 2, 8, rec)
    # ws, ldx, n, w_dim, nl, layers, stream
    check(lib, ["ic2_modconv_prep_batched"], "ic2_modconv_prep_batched", (P(ws), 100, 2, 8, 3, P(rec), STREAM))
    with pytest.raises(TypeError, match="ic2_modconv_prep_batched"):
        ops.modconv_prep_batched(ws, 100, 2, 8, rec.astype(np.int32))
    assert len(lib.calls) == 1


def test_synth_input_and_reparameterize(fake):
    lib = fake()
    t, fr, ph, tr = T(8), T(10), T(5), T(9)
    feats = ops.synth_input_features(t, fr, ph, tr, 2, 5, 32, 9, 16.0, 2.5, BF16)
    assert feats.shape == (2, 9, 9, 32) and feats.dtype == BF16
    # t, freqs, phases, transform, n, c, c_p, size, sampling_rate, bandwidth, out, dtype, stream
    check(lib, ["ic2_synth_input_features"], "ic2_synth_input_features",
          (P(t), P(fr), P(ph), P(tr), 2, 5, 32, 9, 16.0, 2.5, P(feats), nv.BF16, STREAM))
    lib = fake()
    p, eps, w, m, lv = T(2 * 3 * 4 * 2), T(2 * 3 * 4), T(2 * 9 * 4), T(2 * 9 * 4), T(2 * 9 * 4)
    ops.reparameterize(p, eps, 2, 3, 4, 9, 5, w, m, lv)
    # params, eps, n, num_ws, w_dim, ws_total, ws_off, w_out, mean_out, logvar_out, stream
    check(lib, ["ic2_reparameterize"], "ic2_reparameterize", (P(p), P(eps), 2, 3, 4, 9, 5, P(w), P(m), P(lv), STREAM))
    with pytest.raises(ValueError, match="ic2_reparameterize"):
        ops.reparameterize(p, eps, 2, 3, 4, 9, 7, w, m, lv)
    assert len(lib.calls) == 1


def test_quantizers_and_resize(fake):
    lib = fake()
    w, q, idx = T(24), T(24), T(24, torch.int32)
    ops.quantize_uniform(w, 6, q, idx)
    # w, n, bits, q_out, idx_out, stream
    check(lib, ["ic2_quantize_uniform"], "ic2_quantize_uniform", (P(w), 24, 6, P(q), P(idx), STREAM))
    lib = fake()
    img, out = T(6 * 5 * 7), T(6 * 3 * 4)
    ops.resize_bilinear(img, out, 6, 5, 7, 3, 4)
    # img, out, nc, h, w, oh, ow, stream
    check(lib, ["ic2_resize_bilinear"], "ic2_resize_bilinear", (P(img), P(out), 6, 5, 7, 3, 4, STREAM))
    lib = fake()
    z, cb, lt, seed, noise = T(6), T(4), T(1), T(1, torch.int64), T(24)
    disc, ix, ps = T(6), T(6, torch.int64), T(4)
    ops.gumbel_quantize(z, cb, lt, True, seed, noise, disc, ix, ps)
    # z, n, codebook, k, log_tau, tau_scale, hard, seed_dev, offset, noise, disc, idx, psum, stream
    check(lib, ["ic2_gumbel_softmax_quantize_dseed"], "ic2_gumbel_softmax_quantize_dseed",
          (P(z), 6, P(cb), 4, P(lt), 1.0, 1, P(seed), 0, P(noise), P(disc), P(ix), P(ps), STREAM))
    lib = fake(ic2_gumbel_softmax_bwd_ws_bytes=96)
    g, qv = T(6), T(4)
    dz, dlogt = ops.gumbel_quantize_bwd(z, cb, lt, seed, None, g, qv, True)
    assert dz.shape == (6,) and dlogt.shape == (1,)
    # z, n, codebook, k, log_tau, tau_scale, seed_dev, offset, noise, g, q, dz, dlog_tau, ws, ws_bytes, stream
    check(lib, ["ic2_gumbel_softmax_bwd_ws_bytes", "ic2_gumbel_softmax_quantize_bwd"], "ic2_gumbel_softmax_quantize_bwd",
          (P(z), 6, P(cb), 4, P(lt), 1.0, P(seed), 0, None, P(g), P(qv), P(dz), P(dlogt), ANY, 96, STREAM))
    lib = fake()
    dz, dlogt = ops.gumbel_quantize_bwd(z, cb, lt, seed, None, g, None, False)
    assert dlogt is None and lib.calls[-1][1][10:15] == (None, P(dz), None, None, 0)


# ------------------------------------------------------------------ every check raises before anything is recorded
def _short(t):
    return torch.zeros(t.shape[:-1] + (t.shape[-1] - 1,), dtype=t.dtype)


def _strided(t):
    return torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype)[..., ::2]


def _other_dtype(t):
    return t.to(F16 if t.dtype != F16 else F32)


def _elsewhere(t):
    return torch.empty(t.shape, dtype=t.dtype, device="meta")


def _wrapper_calls():
    """name -> (callable(**tensors), {tensor argument: its exactly sized valid value}, arguments whose dtype is free)."""
    rec = np.zeros([1, 16], np.int64)
    g4 = T(2 * 10 * 11 * 32, BF16).view(2, 10, 11, 32)
    return {
        "conv": (lambda **t: ops.conv(t["x"], t["w"], t["y"], nv.F16, 2, 5, 7, 6, 8, 4, (3, 1), 1, oscale=t["oscale"],
                                      bias=t["bias"]),
                 dict(x=T(420, F16), w=T(144, F16), y=T(720, F16), oscale=T(16), bias=T(8)), ("y",)),
        "conv_nchw": (lambda **t: ops.conv(t["x"], t["w"], t["y"], nv.F32, 2, 5, 7, 6, 8, 4, 1, 0, out_layout=nv.NCHW),
                      dict(x=T(420), w=T(48), y=T(280)), ("y",)),
        "conv_grad": (lambda **t: ops.conv(t["x"], t["w"], t["y"], nv.F16, 2, 5, 7, 6, 8, 4, 1, 0, out_code=nv.F16_IEEE),
                      dict(x=T(420, F16), w=T(48, F16), y=T(560, F16)), ()),
        "conv_split": (lambda **t: ops.conv(t["x"], t["w"], t["y"], nv.BF16X3, 2, 5, 7, 9, 8, 4, 1, 0),
                       dict(x=T(420, BF16), w=T(72, BF16), y=T(560)), ("y",)),
        "conv_wino": (lambda **t: ops.conv(t["x"], None, t["y"], nv.F16, 2, 5, 7, 6, 8, 4, 3, 1, wino=lambda: t["u"]),
                      dict(x=T(420, F16), u=T(576, F16), y=T(560, F16)), ("y",)),
        "conv_gn": (lambda **t: ops.conv_gn(t["x"], t["w"], t["y"], nv.F16X2, 2, 5, 7, 12, 8, 4, 3, 1, t["bias"], 4, 1e-5),
                    dict(x=T(420, F16), w=T(864, F16), y=T(560, F16), bias=T(8)), ()),
        "from_rgb_conv": (lambda **t: ops.from_rgb_conv("x3", t["x"], t["w"], t["bias"], t["y"], 2, 5, 7, 3, 20, 32),
                          dict(x=T(210), w=T(540), bias=T(32), y=T(4480, BF16)), ()),
        "from_rgb_conv_bf16": (lambda **t: ops.from_rgb_conv("", t["x"], t["w"], t["bias"], t["y"], 2, 5, 7, 3, 32, 64),
                               dict(x=T(210), w=T(64 * 9 * 32, BF16), bias=T(64), y=T(4480, BF16)), ()),
        "wgrad_oihw": (lambda **t: ops.wgrad_oihw(t["x"], t["dy"], 2, 5, 7, 6, 8, 4, 3, (3, 1), 1),
                       dict(x=T(420, BF16), dy=T(720, BF16)), ("x",)),
        "flrelu": (lambda **t: ops.flrelu(t["x"], t["y"], 2, 32, 9, 11, FU, FD, 2, 2, [1, 1, 1, 1], 1.0, 0.2, -1.0,
                                          post_scale=t["post_scale"]),
                   dict(x=T(5184, F16), y=T(7744, BF16), post_scale=T(64)), ("x", "y")),
        "flrelu_bwd": (lambda **t: ops.flrelu_bwd(t["x"], t["gout"], t["gx"], 2, 32, 9, 9, FU, FD, 2, 2, [1, 1, 1, 1], 1.0,
                                                  0.2, -1.0),
                       dict(x=T(5184, F16), gout=g4, gx=T(5184)), ("x", "gout")),
        "flrelu_bwd_store": (lambda **t: ops.flrelu_bwd(t["x"], g4, t["gx"], 2, 32, 9, 9, FU, FD, 2, 2, [1, 1, 1, 1], 1.0, 0.2,
                                                        -1.0, store=True, mul=t["mul"], bias=t["bias"]),
                             dict(x=T(5184, F16), gx=T(5184, BF16), mul=T(64), bias=T(32)), ("x", "gx")),
        "gn_stats": (lambda **t: ops.gn_stats(t["y"], 2, 35, 32, 30, 4, 1e-5), dict(y=T(2240)), ("y",)),
        "gn_lrelu_pool": (lambda **t: ops.gn_lrelu_pool(t["y"], t["out"], nv.F16, 2, 6, 8, 32, 30, 4, t["stats"],
                                                        t["gamma"], t["beta"], 0.2, True),
                          dict(y=T(3072), out=T(768, F16), stats=T(16), gamma=T(30), beta=T(30)), ("y",)),
        "gn_lrelu_pool_bwd": (lambda **t: ops.gn_lrelu_pool_bwd(t["y"], t["dout"], 2, 6, 8, 32, 30, 4, t["stats"],
                                                                t["gamma"], t["beta"], 0.2, False),
                              dict(y=T(3072), dout=T(3072), stats=T(16), gamma=T(30), beta=T(30)), ("y", "dout")),
        "gap": (lambda **t: ops.gap(t["x"], nv.BF16X3, 2, 35, 32, 30), dict(x=T(4480, BF16)), ()),
        "gap_bwd": (lambda **t: ops.gap_bwd(t["dp"], (2, 5, 7, 32), F16, 30), dict(dp=T(60)), ()),
        "scale": (lambda **t: ops.scale(t["x"], t["xs"], 2, 35, 32), dict(x=T(2240, BF16), xs=T(64)), ("x",)),
        "scale_bwd": (lambda **t: ops.scale_bwd(t["da"], t["x"], t["xs"], 2, 35, 32),
                      dict(da=T(2240, BF16), x=T(2240, BF16), xs=T(64)), ("x",)),
        "to_nhwc": (lambda **t: ops.to_nhwc(t["x"], F16, 32, scale=t["scale"]),
                    dict(x=torch.zeros(2, 3, 5, 7), scale=T(64)), ()),
        "to_nchw": (lambda **t: ops.to_nchw(t["x"], 2, 3, 5, 7, 32), dict(x=T(2240, BF16)), ("x",)),
        "fc": (lambda **t: ops.fc(t["x"], 40, t["w"], t["b"], 2, 5, 7, out=t["out"]),
               dict(x=T(45), w=T(35), b=T(7), out=T(14)), ()),
        "modconv_prep": (lambda **t: ops.modconv_prep(t["st"], t["wsq"], 2, 5, 7, 32, 64, 1, 1.0, 1.0, t["xs"], t["os"]),
                         dict(st=T(10), wsq=T(35), xs=T(64), os=T(128)), ()),
        "modconv_prep_batched": (lambda **t: ops.modconv_prep_batched(t["ws"], 100, 2, 8, rec), dict(ws=T(108)), ()),
        "synth_input_features": (lambda **t: ops.synth_input_features(t["t"], t["fr"], t["ph"], t["tr"], 2, 5, 32, 9, 16.0,
                                                                      2.0, F16),
                                 dict(t=T(8), fr=T(10), ph=T(5), tr=T(9)), ()),
        "reparameterize": (lambda **t: ops.reparameterize(t["p"], t["eps"], 2, 3, 4, 9, 5, t["w"], t["m"], t["lv"]),
                           dict(p=T(48), eps=T(24), w=T(72), m=T(72), lv=T(72)), ()),
        "quantize_uniform": (lambda **t: ops.quantize_uniform(T(24), 8, t["q"], t["idx"]),
                             dict(q=T(24), idx=T(24, torch.int32)), ()),
        "resize_bilinear": (lambda **t: ops.resize_bilinear(t["img"], t["out"], 6, 5, 7, 3, 4),
                            dict(img=T(210), out=T(72)), ()),
        "gumbel_quantize": (lambda **t: ops.gumbel_quantize(T(6), T(4), t["lt"], 0, t["seed"], t["noise"], t["disc"],
                                                            t["idx"], t["psum"]),
                            dict(lt=T(1), seed=T(1, torch.int64), noise=T(24), disc=T(6), idx=T(6, torch.int64),
                                 psum=T(4)), ()),
        "gumbel_quantize_bwd": (lambda **t: ops.gumbel_quantize_bwd(T(6), T(4), t["lt"], None, t["noise"], t["g"], t["q"],
                                                                    True),
                                dict(lt=T(1), noise=T(24), g=T(6), q=T(4)), ()),
    }


_CALLS = _wrapper_calls()
_BREAKS = [("short", _short, ValueError), ("strided", _strided, ValueError), ("dtype", _other_dtype, TypeError),
           ("device", _elsewhere, ValueError)]


@pytest.mark.parametrize("name", sorted(_CALLS))
def test_valid_call_passes_every_check(fake, name):
    lib = fake(ic2_conv_wino_preferred=1)
    fn, tensors, _ = _CALLS[name]
    fn(**tensors)
    assert lib.calls


@pytest.mark.parametrize("name,arg,how", [(n, a, h[0]) for n in sorted(_CALLS) for a in _CALLS[n][1] for h in _BREAKS
                                          if not (h[0] == "dtype" and a in _CALLS[n][2])
                                          and not (h[0] == "short" and n == "to_nhwc" and a == "x")   # its own shape
                                          and not (h[0] == "strided" and _CALLS[n][1][a].numel() == 1)
                                          and not (h[0] == "device" and len(_CALLS[n][1]) == 1)])   # it is the device
def test_bad_tensor_raises_before_any_launch(fake, name, arg, how):
    """One element short, non-contiguous, of another dtype than the code says, or on another device: the wrapper raises
    with the entry point's name and nothing reaches the library (queries included, except conv's Winograd rule)."""
    lib = fake(ic2_conv_wino_preferred=1)
    fn, tensors, _ = _CALLS[name]
    brk, exc = next((b, e) for h, b, e in _BREAKS if h == how)
    bad = dict(tensors, **{arg: brk(tensors[arg])})
    with pytest.raises(exc, match="ic2_"):
        fn(**bad)
    assert [c[0] for c in lib.calls if c[0] != "ic2_conv_wino_preferred"] == []


def test_missing_required_tensor_and_bad_filters(fake):
    lib = fake()
    with pytest.raises(ValueError, match="ic2_conv3x3_gn_fwd: bias is required"):
        ops.conv_gn(T(420, BF16), T(432, BF16), T(560, BF16), nv.BF16, 2, 5, 7, 6, 8, 4, 3, 1, None, 4, 1e-5)
    with pytest.raises(ValueError, match="ic2_conv_igemm_ws: w is required"):
        ops.conv(T(420), None, T(280), nv.F32, 2, 5, 7, 6, 8, 4, 1, 0, out_layout=nv.NCHW)
    x, y = T(5184), T(7744)
    for fu, fd, radial in ((FU.astype(np.float64), FD, None), (FU[::2], FD, None), (FU, FD, (3, FDV, FDH)),
                           (FU, FD2, (2, FDV, FDH)), (FU, np.zeros([12, 8], np.float32), (0, None, None))):
        with pytest.raises(TypeError, match="ic2_flrelu_nhwc"):
            ops.flrelu(x, y, 2, 32, 9, 11, fu, fd, 2, 2, [1, 1, 1, 1], 1.0, 0.2, -1.0, radial=radial)
    with pytest.raises(ValueError, match="ic2_flrelu_bwd_nhwc: fu is required"):
        ops.flrelu_bwd(x, T(7744).view(2, 11, 11, 32), T(5184), 2, 32, 9, 9, None, FD, 2, 2, [1, 1, 1, 1], 1.0, 0.2, -1.0)
    assert lib.calls == []


# ------------------------------------------------------------------ _native.try_call
def test_try_call_goes_through_call(fake, monkeypatch):
    lib = fake(ic2_x=2, ic2_y=1)
    seen = []
    orig = nv.call

    def spy(name, *args):
        seen.append((name, args))
        return orig(name, *args)
    monkeypatch.setattr(nv, "call", spy)
    assert nv.try_call("ic2_ok", 1, 2.5) is True
    assert nv.try_call("ic2_x", 3) is False
    with pytest.raises(RuntimeError, match="ic2_y failed .code 1.: fake message") as e:
        nv.try_call("ic2_y", 4)
    assert e.value.code == 1
    assert seen == [("ic2_ok", (1, 2.5)), ("ic2_x", (3,)), ("ic2_y", (4,))]
    assert lib.calls == [("ic2_ok", (1, 2.5)), ("ic2_x", (3,)), ("ic2_y", (4,))]
    with pytest.raises(RuntimeError) as e:
        nv.call("ic2_x")
    assert e.value.code == nv.E_UNSUPPORTED == 2
