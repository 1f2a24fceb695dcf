"""The filtered-lrelu FORWARD kernels per element at edge geometries: the strip kernel (flrelu_mfma3_kernel, f16 input,
16-row x 32-column strips), the tile kernel (flrelu_mfma_kernel, bf16 input, 16 x 16 tiles) and the VALU kernel
(flrelu_kernel: bf16 NHWC with a bias on 16 x 16 tiles; f32 NHWC and f32 / bf16 NCHW on 24 x 8 tiles), against the fp64
reference of tests/flrelu_fwd_oracle.py (pinned by tests/test_flrelu_fwd_oracle_host.py).  Every call goes through
the C ABI with the output NaN-prefilled between sentinel guard bands, and every element must satisfy

    |got - ref| <= K eps_op B + eps_out |ref| + F

(B the magnitude bound, F the f16 subnormal floor, eps_op / eps_out the unit roundoffs: the oracle's docstring).  Taps
are asymmetric, down is 2 with 12 taps.  Two tiers per geometry: `linear` (slope 1, no clamp, Gaussian x 3: the
instance without the clamp split) and `mask` (slope 0.2, clamp 256, the first third of the channels at std 300: the
clamp-split instance on the strip kernel).

K per path: derived (the count in the oracle's docstring) / measured / bar.  Measured is the largest
|got - ref| / (eps_op B) over the runs of this file whose output format is no coarser than the operands (f16 out on the
MFMA kernels, f32 / bf16 out on the f32 / bf16 VALU instances): it contains the output rounding, which the bound
allows separately.  A bf16 output on the MFMA kernels is left out of the measure, its own rounding is 8 eps_op
(measured with it: 5.89 strip, 5.30 tile); the bound keeps it as eps_out and those runs are held to the same bar.
The bar is at least 1.5 x measured (one seed per case) and never above derived; the figures and where the maxima
occur are recorded in profiles/r19_flr_fwd_edges.txt:

  mfma_strip  derived 14 (16 clamp-split)   measured 1.48 (linear), 1.23 (mask)   bar 2.5
  mfma_tile   derived 14                    measured 1.17 (linear), 1.19 (mask)   bar 2.5
  valu_f32    derived 29                    measured 2.64 (linear), 2.36 (mask)   bar 4
  valu_bf16   derived 2.1                   measured 0.94 (linear), 0.84 (mask)   bar 1.5
"""
import ctypes

import numpy as np
import pytest
import torch

import flrelu_bwd_oracle as fo
import flrelu_fwd_oracle as fw
from image_compression_2_amd import _native as nv

pytestmark = pytest.mark.gpu

GUARD = 8192
SENTINEL = -1536.0  # exact in f16, bf16 and f32
F32, BF16, F16 = fw.F32, fw.BF16, fw.F16
K_BAR = {"mfma_strip": 2.5, "mfma_tile": 2.5, "valu_f32": 4.0, "valu_bf16": 1.5}
INVALID, UNSUPPORTED = 1, 2
RATIOS = {}


def _guarded(shape, dtype, dev):
    """A NaN-filled tensor of `shape` inside a buffer with sentinel guard bands -> (buffer, view)."""
    numel = int(np.prod(shape))
    base = torch.full([GUARD + numel + GUARD], SENTINEL, device=dev, dtype=dtype)
    base[GUARD:GUARD + numel] = float("nan")
    y = base[GUARD:GUARD + numel].view(shape)
    assert y.data_ptr() % 16 == 0
    return base, y


def _guards_intact(base, numel):
    return bool((base[:GUARD] == SENTINEL).all() and (base[GUARD + numel:] == SENTINEL).all())


def _fp(t):
    a = t.float().contiguous().numpy()
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _block(x):
    """NHWC [n, h, w, c_p] -> channel-blocked NHWC16 [n, c_p / 16, h, w, 16]."""
    n, h, w, cp = x.shape
    return x.reshape(n, h, w, cp // 16, 16).permute(0, 3, 1, 2, 4).contiguous()


def _unblock(y):
    n, cb, h, w, _ = y.shape
    return y.permute(0, 2, 3, 1, 4).reshape(n, h, w, cb * 16)


def run_fwd(dev, x, odt, fu, fd, up, pad, slope, clamp, flip, bias=None, ps=None, entry="nhwc", blocked_out=False,
            out_hw=None, on_device=False):
    """One call of ic2_flrelu_nhwc / ic2_flrelu_nhwc16 / ic2_filtered_lrelu on x (NHWC [n, h, w, c_p], stored dtype; a
    tensor already on the device is used as is) -> (rc, y as NHWC, NaN-prefilled between guard bands that are asserted
    intact).  entry nhwc16 blocks the input first; blocked_out asks for NHWC16 and un-blocks the result."""
    n, h, w, cp = x.shape
    oh, ow = fo.out_size(h, w, up, pad) if out_hw is None else out_hw
    xd = x.to(dev)
    xs = _block(xd) if entry == "nhwc16" else (xd.permute(0, 3, 1, 2).contiguous() if entry == "nchw" else xd.contiguous())
    bd = None if bias is None else bias.to(dev)
    pd = None if ps is None else ps.to(dev).contiguous()
    shape = [n, cp // 16, oh, ow, 16] if blocked_out else ([n, cp, oh, ow] if entry == "nchw" else [n, oh, ow, cp])
    base, y = _guarded(shape, odt, dev)
    fua, fup = _fp(fu)
    fda, fdp = _fp(fd)
    lib = nv.load()
    if entry == "nchw":
        assert odt == x.dtype and ps is None
        rc = lib.ic2_filtered_lrelu(nv.ptr(xs), nv.ptr(y), nv.dtype_code(odt), n, cp, h, w, oh, ow, fup, fua.shape[0], fdp,
                                    fda.shape[0], nv.ptr(bd), up, 2, *pad, float(fo.GAIN), slope, clamp, int(flip),
                                    nv.stream_of(xs))
    else:
        code = nv.dtype_code(odt) | (nv.flr_out_layout(nv.NHWC16) if blocked_out else 0)
        rc = getattr(lib, "ic2_flrelu_" + entry)(nv.ptr(xs), nv.ptr(y), nv.dtype_code(x.dtype), code, n, cp, h, w, oh, ow,
                                                  fup, fua.shape[0], fdp, fda.shape[0], nv.ptr(bd), up, 2, *pad,
                                                  float(fo.GAIN), slope, clamp, int(flip), nv.ptr(pd), nv.stream_of(xs))
    torch.cuda.synchronize()
    del fua, fda
    assert _guards_intact(base, y.numel()), "store outside the output"
    out = _unblock(y) if blocked_out else (y.permute(0, 2, 3, 1) if entry == "nchw" else y)
    return rc, (out if on_device else out.cpu())


def check(got, r, key, tier, odt, F, c, tag):
    """The per-element bound of the module docstring; prints the measured ratio, then asserts."""
    g = got.double()
    assert torch.isfinite(g).all(), f"{tag}: output not written everywhere"
    assert (g[..., c:] == 0).all(), f"{tag}: padded channels"
    eps = fw.EPS_OP[key]
    err = (g[..., :c] - r["ref"]).abs()
    bound = fw.bound(r, K_BAR[key], eps, odt, F)
    live = r["B"] > 0
    ratio = ((err - fw.EPS_OUT[odt] * r["ref"].abs() - F).clamp_min(0)[live] / (eps * r["B"][live])).max().item()
    raw = (err[live] / (eps * r["B"][live])).max().item()
    if fw.EPS_OUT[odt] <= eps:
        RATIOS[key, tier] = max(RATIOS.get((key, tier), 0.0), raw)
    bad = err > bound
    print(f"[flrelu-fwd-edges] {tag} {key} {tier} -> {str(odt).split('.')[-1]}: max err/(eps B) {raw:.3f} (less the "
          f"output rounding and F {ratio:.3f}), over the bound {int(bad.sum())} of {bad.numel()}"
          + (f", worst err/bound {(err / bound.clamp_min(1e-300))[bad].max().item():.2f}" if bad.any() else ""))
    assert live.any()
    assert not bad.any(), f"{tag}: {int(bad.sum())} elements over the bound, first at {bad.nonzero()[0].tolist()}"


def run_case(dev, tag, path, x, b, ps, c, odt, up, pad, tier, flip, blocked_in=False, blocked_out=False, kw=None):
    """Run one call and check every element against the reference of the same stored operands -> y (NHWC, host)."""
    fu, fd = fo.taps(up)
    kw = fw.TIERS[tier] if kw is None else kw
    entry = "nchw" if path == "nchw" else ("nhwc16" if blocked_in else "nhwc")
    rc, got = run_fwd(dev, x, odt, fu, fd, up, pad, kw["slope"], kw["clamp"], flip, b, ps, entry, blocked_out)
    assert rc == 0, nv.load().ic2_last_error().decode()
    r = fw.forward_reference(x, fu, fd, up, pad, flip=flip, bias=b, post_scale=ps, c=c, **kw)
    F = fw.floor_f16(path, fu, fd, up, fo.GAIN, kw["clamp"], ps, odt, x.dtype, x.shape[0], c)
    check(got, r, fw.key_of(path, x.dtype), tier, odt, F, c, tag)
    return got, r


# ------------------------------------------------------------------ the geometry sweep
SWEEP = [c for p in fw.PATHS for c in fw.sweep_cases(p)]


@pytest.mark.parametrize("case", SWEEP, ids=[f"{c['path']}-{c['id']}" for c in SWEEP])
def test_flrelu_fwd_edge_geometry(cuda, case):
    """Every geometry of the table on its path, both tiers; flip, the strip kernel's input layout and the NCHW dtype
    alternate by case.  The MFMA kernels write bf16 in one tier and f16 in the other (which one alternates by case),
    the VALU instances their input dtype."""
    path, i = case["path"], SWEEP.index(case)
    for j, tier in enumerate(("linear", "mask")):
        x, b, ps, c = fw.case_inputs(case, tier)
        odt = (BF16, F16)[(i + j) % 2] if path in ("strip", "tile") else x.dtype
        run_case(cuda, f"{path} {case['id']} flip {case['flip']}", path, x, b, ps, c, odt, case["up"], case["pad"], tier,
                 case["flip"], blocked_in=case["blocked_in"])


# ------------------------------------------------------------------ dtype and layout matrix
def _matrix_case(up, path, xdt):
    name, h, w = fw.MATRIX[up]
    return dict(id=f"{name}-{h}x{w}", path=path, up=up, pad=fw.PADS[name][1], in_h=h, in_w=w, flip=up // 4, xdt=xdt,
                blocked_in=False)


MFMA_COMBOS = [("strip", F16, odt, bi, bo) for odt in (BF16, F16) for bi in (0, 1) for bo in (0, 1)] + \
              [("tile", BF16, odt, bi, 0) for odt in (BF16, F16) for bi in (0, 1)]


@pytest.mark.parametrize("path,xdt,odt,bin_,bout", MFMA_COMBOS,
                         ids=[f"{p}-{str(o).split('.')[-1]}-in{'16' if bi else ''}-out{'16' if bo else ''}"
                              for p, _, o, bi, bo in MFMA_COMBOS])
@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_fwd_mfma_dtype_layout_matrix(cuda, up, path, xdt, odt, bin_, bout):
    """Every (output dtype, input layout, output layout) the MFMA entry points accept: strip f16 -> bf16 / f16 with
    NHWC or NHWC16 on either side; tile bf16 -> bf16 / f16 with NHWC or NHWC16 input.  Both tiers."""
    case = _matrix_case(up, path, xdt)
    for tier in ("linear", "mask"):
        x, b, ps, c = fw.case_inputs(case, tier)
        run_case(cuda, f"{path} {case['id']}", path, x, b, ps, c, odt, up, case["pad"], tier, case["flip"],
                 blocked_in=bool(bin_), blocked_out=bool(bout))


@pytest.mark.parametrize("path,xdt", [("valu16", BF16), ("valu24", F32), ("nchw", F32), ("nchw", BF16)],
                         ids=["bf16_nhwc", "f32_nhwc", "f32_nchw", "bf16_nchw"])
@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_fwd_valu_dtype_matrix(cuda, up, path, xdt):
    """The VALU instances behind the entry points: bf16 and f32 NHWC with a bias and a post_scale, f32 and bf16 NCHW
    with c = 19 and a bias.  Both tiers, and the opposite flip of the sweep's matrix geometry."""
    case = _matrix_case(up, path, xdt)
    for tier in ("linear", "mask"):
        x, b, ps, c = fw.case_inputs(case, tier)
        run_case(cuda, f"{path} {case['id']}", path, x, b, ps, c, xdt, up, case["pad"], tier, 1 - case["flip"])


@pytest.mark.parametrize("path,xdt", [("strip", F16), ("tile", BF16)])
@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_fwd_blocked_input_bit_identical(cuda, up, path, xdt):
    """ic2_flrelu_nhwc16 on the channel-blocked copy gives the bits of ic2_flrelu_nhwc, on both MFMA kernels and for
    either output layout of the strip kernel (each run is also within the bound)."""
    case = _matrix_case(up, path, xdt)
    for tier in ("linear", "mask"):
        x, b, ps, c = fw.case_inputs(case, tier)
        for bout in ((False, True) if path == "strip" else (False,)):
            y0, _ = run_case(cuda, f"{path} nhwc", path, x, b, ps, c, BF16, up, case["pad"], tier, 0, False, bout)
            y1, _ = run_case(cuda, f"{path} nhwc16", path, x, b, ps, c, BF16, up, case["pad"], tier, 0, True, bout)
            assert torch.equal(y0, y1)


@pytest.mark.parametrize("path,xdt", [("strip", F16), ("tile", BF16), ("valu16", BF16), ("valu24", F32)])
@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_fwd_null_post_scale_and_wide_clamp(cuda, up, path, xdt):
    """post_scale NULL (mask tier), and clamp 1e4: lim = clamp / gain > 4096 takes the strip kernel off the clamp
    split, so the plain activation runs with a finite clamp (input x 20, below the f16 range, so that the clamp is
    reached: on 0.3 % of the grid of the clamp channels at up 2, 7 % at up 4)."""
    case = _matrix_case(up, path, xdt)
    x, b, ps, c = fw.case_inputs(case, "mask")
    run_case(cuda, f"{path} null post_scale", path, x, b, None, c, F16 if path in ("strip", "tile") else xdt, up, case["pad"],
             "mask", 1)
    kw = dict(slope=0.2, clamp=1e4)
    assert not fw.clamp_split(path, kw["clamp"])
    x20 = (x.double() * 20).to(xdt)
    _, r = run_case(cuda, f"{path} clamp 1e4", path, x20, b, ps, c, F16 if path in ("strip", "tile") else xdt, up,
                    case["pad"], "mask", 0, kw=kw)
    assert r["clamped"][: c // 3].mean().item() > 0.001


# ------------------------------------------------------------------ replicated cases: chained strips, persistent tiles
def run_replicated(dev, path, up, pad, in_h, in_w, n, c_p, tier, odt, blocked_in, blocked_out, seed, tag):
    """One sample of 16 channels replicated to n x c_p channels, each (sample, 16-channel block) copy scaled by a
    power of two (fw.scale_index) and every (sample, channel) with its own post_scale.  The reference is computed in
    fp64 over the 16 channels once per distinct scale and expanded on the device, where every element of the output
    is checked against the bound."""
    xdt = F16 if path == "strip" else BF16
    fu, fd = fo.taps(up)
    kw = fw.TIERS[tier]
    cb = c_p // 16
    x1, ps, idx = fw.replicated_inputs(up, tier, in_h, in_w, n, c_p, xdt, seed)
    copies = [(x1 * s).to(xdt) for s in fw.SCALES]                       # [1, h, w, 16] each, as stored
    refs = [fw.forward_reference(xc, fu, fd, up, pad, flip=0, c=16, **kw) for xc in copies]
    idx_d = idx.to(dev)
    xs = torch.stack([xc[0] for xc in copies]).to(dev)[idx_d]            # [n, cb, h, w, 16]
    x = xs.permute(0, 2, 3, 1, 4).reshape(n, in_h, in_w, c_p)
    rc, got = run_fwd(dev, x, odt, fu, fd, up, pad, kw["slope"], kw["clamp"], 0, None, ps,
                      "nhwc16" if blocked_in else "nhwc", blocked_out, on_device=True)
    assert rc == 0, nv.load().ic2_last_error().decode()
    oh, ow = got.shape[1:3]
    psd = ps.double().to(dev).view(n, 1, 1, cb, 16)

    def expand(key):
        t = torch.stack([r[key][0] for r in refs]).to(dev)[idx_d]        # [n, cb, oh, ow, 16]
        return t.permute(0, 2, 3, 1, 4)
    ref, B = expand("ref") * psd, expand("B") * psd.abs()
    F = fw.floor_f16(path, fu, fd, up, fo.GAIN, kw["clamp"], ps, odt, xdt, n, c_p).to(dev).view(n, 1, 1, cb, 16)
    g = got.double().view(n, oh, ow, cb, 16)
    assert torch.isfinite(g).all(), f"{tag}: output not written everywhere"
    key = fw.KEY[path]
    eps = fw.EPS_OP[key]
    err = (g - ref).abs()
    bound = K_BAR[key] * eps * B + fw.EPS_OUT[odt] * ref.abs() + F
    live = B > 0
    ratio = ((err - fw.EPS_OUT[odt] * ref.abs() - F).clamp_min(0)[live] / (eps * B[live])).max().item()
    raw = (err[live] / (eps * B[live])).max().item()
    if fw.EPS_OUT[odt] <= eps:
        RATIOS[key, tier] = max(RATIOS.get((key, tier), 0.0), raw)
    bad = err > bound
    print(f"[flrelu-fwd-edges] {tag} {key} {tier} -> {str(odt).split('.')[-1]}: {n * cb} blocks of {oh} x {ow}, max "
          f"err/(eps B) {raw:.3f} (less the output rounding and F {ratio:.3f}), over the bound {int(bad.sum())} of "
          f"{bad.numel()}")
    assert live.any()
    assert not bad.any(), f"{tag}: {int(bad.sum())} elements over the bound, first at {bad.nonzero()[0].tolist()}"


CHAIN_COMBOS = [(BF16, False), (F16, True), (F16, False), (BF16, True)]   # (output dtype, blocked output)


@pytest.mark.parametrize("k", range(3), ids=[f"out_h{h}" for h in fw.CHAIN_OUT_H])
@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_fwd_strip_chained(cuda, up, k):
    """2048 strips of 3 / 4 / 5 tiles (last tile with 11 or 10 / 12 / 16 live rows): fm_strip_segments keeps whole
    strips and every workgroup takes several, so the ring hand-over between blocks, the counted store waits of k >= 3,
    the next item's prefetch and the accumulator swap run (tests/test_flrelu_fwd_oracle_host.py evaluates the
    segmentation).  The six (height, tier) runs of one up factor cover bf16 / f16 and NHWC / NHWC16 output and both
    input layouts."""
    in_h, oh = fw.chain_in_h(up, fw.CHAIN_OUT_H[k])
    for j, tier in enumerate(("linear", "mask")):
        odt, bout = CHAIN_COMBOS[(2 * k + j) % 4]
        run_replicated(cuda, "strip", up, fw.CHAIN_PAD[up], in_h, fw.CHAIN_W, fw.CHAIN_N, fw.CHAIN_CP, tier, odt,
                       blocked_in=(k + j) % 2 == 1, blocked_out=bout, seed=40, tag=f"chained u{up} out_h {oh}")


@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_fwd_tile_persistent(cuda, up):
    """4096 tiles on the persistent tile kernel (more than its resident workgroups: each walks several tiles)."""
    pad, in_h, in_w = fw.PERSIST[up]
    oh, ow = fo.out_size(in_h, in_w, up, pad)
    assert fw.PERSIST_N * -(-oh // 16) * -(-ow // 16) * (fw.PERSIST_CP // 16) >= 4096
    for j, tier in enumerate(("linear", "mask")):
        run_replicated(cuda, "tile", up, pad, in_h, in_w, fw.PERSIST_N, fw.PERSIST_CP, tier, (F16, BF16)[j],
                       blocked_in=j == 1, blocked_out=False, seed=60, tag=f"persistent u{up} {oh}x{ow}")


# ------------------------------------------------------------------ the entry point's refusals
@pytest.mark.parametrize("what", ["blocked_out_bf16_in", "f16_bias", "phase", "out_size", "taps10_blocked_out"])
def test_flrelu_fwd_refusals_write_nothing(cuda, what):
    """Each refusal returns its code and a message before any launch: the output keeps its NaN prefill."""
    up, pad, h, w = 2, [9, 8, 9, 8], 19, 35
    fu, fd = fo.taps(up)
    xdt, bias, bout, code, out_hw = F16, None, False, UNSUPPORTED, None
    ps, b = fo.scale_bias(2, fo.C, fo.C_P, 3)
    if what == "blocked_out_bf16_in":
        xdt, bout = BF16, True
    elif what == "f16_bias":
        bias = b
    elif what == "phase":
        pad = [9, 8, 10, 7]   # same output size: only the px0 == py0 (mod up) rule objects
    elif what == "out_size":
        oh, ow = fo.out_size(h, w, up, pad)
        out_hw, code = (oh + 1, ow), INVALID
    elif what == "taps10_blocked_out":
        fd, bout = fd[:10].contiguous(), True
        out_hw = (h - 1, w - 1)   # (2 in + 17 - 11 - 9 + 1) / 2 with 10 down taps
    x = fo.gauss(2, h, w, fo.C, fo.C_P, 1, xdt)
    rc, got = run_fwd(cuda, x, BF16, fu, fd, up, pad, 0.2, 256.0, 0, bias, ps, "nhwc", bout, out_hw)
    msg = nv.load().ic2_last_error().decode()
    assert rc == code, (rc, msg)
    assert "flrelu_nhwc" in msg
    assert torch.isnan(got.float()).all()


def test_zz_report_measured_ratios():
    """Prints the largest |got - ref| / (eps_op B) each path and tier reached over the cases above (the `measured` of
    the module docstring); no bar exceeds its derived count."""
    for (key, tier), v in sorted(RATIOS.items()):
        print(f"[flrelu-fwd-edges measured] {key} {tier}: {v:.3f}, bar {K_BAR[key]}, derived {fw.K_DERIVED[key]}")
    assert all(K_BAR[k] <= fw.K_DERIVED[k] for k in K_BAR)
