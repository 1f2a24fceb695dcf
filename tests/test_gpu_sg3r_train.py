"""GPU: training through a StyleGAN3-R generator.  ic2_flrelu_bwd_nhwc_2d (csrc/flrelu_radial_bwd.hip: the filtered
lrelu's backward with a 12 x 12 non-separable down filter) per element against the fp64 reference of
tests/flrelu_bwd_oracle.py on the cases of tests/sg3r_bwd_cases.py (pinned on the CPU by tests/test_sg3r_bwd_host.py),
then the layer, the network, the training step and the opt-in switch Generator.set_radial_training.

Kernel scheme (that of tests/test_gpu_flrelu_bwd_edges.py, restated): every call goes through the C ABI with gx and
ydot NaN-prefilled between sentinel guard bands; per element, with B (magnitude bound) and A (mask allowance) from
the oracle,

  linear  slope 1, no clamp: |got - ref| <= K eps B + eps_out |ref|
  mask    slope 0.2, clamp 256 on block-sign inputs: the same plus A, and A > 0 on at most 20 % of the elements

eps = 2^-24 in every instance: the kernel does f32 arithmetic on the stored operands and keeps every intermediate of
the gradient chain (the gout window, gV, gU, the horizontal pass) as f32 in LDS, whatever the storage dtypes.  For
the same reason eps_x (the unit of the U recompute, for A) is 2^-24 in every instance.  eps_out is the unit roundoff
of the stored gx (2^-8 bf16, 2^-11 f16, 2^-24 f32); an f16 gx below the smallest normal f16 (2^-14: the border
elements of the up-4 crops, which few taps reach) is rounded to the subnormal spacing 2^-24, so there the output term is
2^-25 instead of eps_out |ref|.

K: derived 88 = the roundings of the chain as built, for up 4: 36 FMAs of the gather, 2 for the mask factor (gain *
slope, then the product), 24 + 24 FMAs of the two separable down-by-up passes (every one of the 6 up taps of the 4
phases reaches an output), 1 for the oscale product, 1 for gain = sqrt(2) passed as f32 (up 2: 12 + 12 taps, 64).
Measured on MI355X over all cases of this file, max |got - ref| / (eps B) on the f32-output instances: 2.84
(linear), 3.47 (mask).  Bar K_BAR = 6.9 <= min(derived, 2 x measured).  Recorded in profiles/r17_sg3r_train.txt.
"""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flrelu_bwd_oracle as fo
import image_compression_2_amd as ic2
import sg3r_bwd_cases as sc
import sg3r_oracle as so
from image_compression_2_amd import _native as nv
from image_compression_2_amd import autograd_ops as ao
from image_compression_2_amd import training as ict
from oracle import sg3

pytestmark = pytest.mark.gpu

GUARD = 8192
SENTINEL = -1536.0  # exact in f16, bf16 and f32
F32, BF16, F16 = sc.F32, sc.BF16, sc.F16
EPS = 2.0 ** -24
EPS_OUT = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}
F16_TINY = 2.0 ** -14   # smallest normal f16: below it the spacing is 2^-24 whatever the value
K_DERIVED = 88.0
K_BAR = 6.9
INVALID, UNSUPPORTED = 1, 2
C, C_P = sc.C, sc.C_P
_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}


# ------------------------------------------------------------------ the kernel through the C ABI
def _guarded(shape, dtype, dev):
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


def run_bwd(dev, x, gout, odt, fu, fd, up, pad, slope, clamp, flip, oscale=None, bias=None, want_ydot=True,
            out_hw=None, ydot_short=0, fd_taps=12, fu_taps=None):
    """One call of ic2_flrelu_bwd_nhwc_2d -> (rc, gx on the host, ydot on the host or None)."""
    n, h, w, cp = x.shape
    oh, ow = gout.shape[1:3] if out_hw is None else out_hw
    xd, gd = x.to(dev), gout.to(dev)
    osd = None if oscale is None else oscale.to(dev)
    bd = None if bias is None else bias.to(dev)
    gbase, gx = _guarded([n, h, w, cp], odt, dev)
    nyd = int(nv.query("ic2_flrelu_bwd_2d_ydot_floats", n, cp, h, w, up))
    ty, tx = sc.TILE.get(up, (16, 16))
    assert nyd == n * -(-h // ty) * -(-w // tx) * cp
    ybase, yd = _guarded([nyd], F32, dev) if want_ydot else (None, None)
    fua, fup = _fp(fu)
    fda, fdp = _fp(fd)
    assert fda.shape == (12, 12)
    rc = nv.load().ic2_flrelu_bwd_nhwc_2d(
        nv.ptr(xd), nv.dtype_code(x.dtype), nv.ptr(gd), nv.dtype_code(gout.dtype), nv.ptr(gx), nv.dtype_code(odt), n, cp,
        h, w, oh, ow, fup, fua.shape[0] if fu_taps is None else fu_taps, fdp, fd_taps, up, 2, *pad, float(fo.GAIN), slope,
        clamp, int(flip), nv.ptr(osd), nv.ptr(bd), nv.ptr(yd), nyd - ydot_short if want_ydot else 0, nv.stream_of(xd))
    torch.cuda.synchronize()
    assert _guards_intact(gbase, gx.numel()), "store outside gx"
    if want_ydot:
        assert _guards_intact(ybase, nyd), "store outside ydot"
    return rc, gx.cpu(), (yd.cpu() if want_ydot else None)


RATIOS = {}


def check_gx(got, r, odt, tier, tag):
    """The per-element bound of the module docstring; prints the measured ratio, then asserts."""
    g = got.double()
    assert torch.isfinite(g).all(), f"{tag}: gx not written everywhere"
    assert (g[..., C:] == 0).all(), f"{tag}: padded channels of gx"
    assert (g[..., :C][r["B"] == 0] == 0).all(), f"{tag}: elements no gout term reaches must be exactly 0"
    err = (g[..., :C] - r["ref"]).abs()
    out_term = EPS_OUT[odt] * r["ref"].abs()
    if odt == F16:
        out_term = torch.where(r["ref"].abs() < F16_TINY, torch.full_like(out_term, 2.0 ** -25), out_term)
    bound = K_BAR * EPS * r["B"] + out_term + (r["A"] if tier == "mask" else 0.0)
    clean = (r["A"] == 0) & (r["B"] > 0)
    raw = (err[clean] / (EPS * r["B"][clean])).max().item()
    less = ((err - out_term).clamp_min(0)[clean] / (EPS * r["B"][clean])).max().item()
    if odt == F32:
        RATIOS[tier] = max(RATIOS.get(tier, 0.0), raw)
    share = (r["A"] > 0).double().mean().item()
    bad = err > bound
    print(f"[sg3r-bwd] {tag} {tier}: max err/(eps B) {raw:.3f} (less the output rounding {less:.3f}), "
          f"A > 0 on {100 * share:.1f} %, over the bound {int(bad.sum())} of {bad.numel()}"
          + (f", worst err/bound {(err / bound.clamp_min(1e-300))[bad].max().item():.2f}" if bad.any() else ""))
    if tier == "mask":
        assert share <= 0.20, f"{tag}: mask allowance on {100 * share:.1f} % of the elements"
    else:
        assert r["A"].abs().max().item() == 0.0
    assert (r["B"] > 0).any()
    assert not bad.any(), f"{tag}: {int(bad.sum())} elements over the bound, first at {bad.nonzero()[0].tolist()}"


def check_ydot(yd, r, up, tier, tag):
    """ydot [n][tile][c_p]: every tile's partial (partial tiles included) against the reference restricted to that
    tile.  Bound (check_ydot_valu's): the gx bound (unscaled) times |x - bias| summed over the tile, plus the f32
    accumulation of the tile's products (2^-24 each, tile size + 2 roundings at the most) on the sum of magnitudes."""
    n, h, w, _ = r["ref0"].shape
    th, tw = sc.TILE[up]
    ty, tx = -(-h // th), -(-w // tw)
    y = yd.view(n, ty * tx, -1).double()
    assert torch.isfinite(y).all() and (y[..., C:] == 0).all(), tag
    xb = r["x"] - r["bias"]
    per = K_BAR * EPS * r["B0"] + (r["A0"] if tier == "mask" else 0.0)
    worst = 0.0
    for j in range(ty):
        for i in range(tx):
            sl = (slice(None), slice(th * j, th * j + th), slice(tw * i, tw * i + tw))
            ref = (r["ref0"][sl] * xb[sl]).sum(dim=(1, 2))
            tol = ((per[sl] * xb[sl].abs()).sum(dim=(1, 2))
                   + (th * tw + 2) * 2.0 ** -24 * (r["ref0"][sl] * xb[sl]).abs().sum(dim=(1, 2)))
            e = (y[:, j * tx + i, :C] - ref).abs()
            worst = max(worst, (e / tol.clamp_min(1e-300)).max().item())
            assert (e <= tol).all(), f"{tag}: ydot of tile ({j}, {i}) off by {(e / tol.clamp_min(1e-300)).max().item():.2f} bounds"
    print(f"[sg3r-bwd] {tag} ydot: {ty * tx} tiles, worst err/bound {worst:.3f}")


def run_case(dev, geo, which, tier, flip, triple, oscale=True, bias=True, want_ydot=True):
    gid, up, pad, h, w = geo
    xdt, gdt, odt = triple
    fu, fd = sc.filters(up, which)
    x, gout, os_, b = sc.case_inputs(gid, up, pad, h, w, tier, xdt, gdt)
    os_, b = (os_ if oscale else None), (b if bias else None)
    kw = fo.TIERS[tier]
    tag = f"{gid} {which} {_NAME[xdt]}/{_NAME[gdt]}/{_NAME[odt]} flip {flip}"
    rc, got, yd = run_bwd(dev, x, gout, odt, fu, fd, up, pad, kw["slope"], kw["clamp"], flip, os_, b, want_ydot)
    assert rc == 0, nv.load().ic2_last_error().decode()
    r = sc.reference((gid, which, tier, flip, xdt, gdt, oscale, bias), x, gout, fu, fd, up, pad, tier, flip, os_, b)
    check_gx(got, r, odt, tier, tag)
    if want_ydot:
        check_ydot(yd, r, up, tier, tag)
    return got, yd, r


GEOS_R = sc.geometries(("r",))
GEOS_PH = sc.geometries(("ph",))
TRIPLE_IDS = ["f32", "f16_bf16", "f16_f16", "f16_f32"]


@pytest.mark.parametrize("triple", sc.TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("geo", GEOS_R, ids=[g[0] for g in GEOS_R])
def test_kernel_r_paddings_every_instance(cuda, geo, triple):
    """Every dtype triple on the R layers' paddings: non-symmetric filters, the linear tier with flip 0 and the mask
    tier with flip 1, oscale, bias and ydot set, two samples with different data."""
    run_case(cuda, geo, "nonsym", "linear", 0, triple)
    run_case(cuda, geo, "nonsym", "mask", 1, triple)


@pytest.mark.parametrize("geo", GEOS_PH, ids=[g[0] for g in GEOS_PH])
def test_kernel_other_gout_phase_f32(cuda, geo):
    """The paddings of the other gout phase (the kernel's second polyphase instance), f32, both flips in both tiers."""
    for tier in ("linear", "mask"):
        for flip in (0, 1):
            run_case(cuda, geo, "nonsym", tier, flip, sc.TRIPLES[0])


REAL_GEO = {2: [g for g in GEOS_R if g[0] == "u2-r-17x33"][0], 4: [g for g in GEOS_R if g[0] == "u4-r-16x21"][0]}


@pytest.mark.parametrize("triple", sc.TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("up", [2, 4])
def test_kernel_real_r256_filters(cuda, up, triple):
    """The real R-256 designs of L0_36_1024 (up 2) and L3_52_1024 (up 4), every instance, mask tier."""
    run_case(cuda, REAL_GEO[up], "r256", "mask", 0, triple)


@pytest.mark.parametrize("null", ["oscale", "bias", "ydot"])
def test_kernel_null_arguments(cuda, null):
    run_case(cuda, REAL_GEO[2], "nonsym", "mask", 0, sc.TRIPLES[0], oscale=null != "oscale", bias=null != "bias",
             want_ydot=null != "ydot")


@pytest.mark.parametrize("up", [2, 4])
def test_kernel_f16_gradient_overflow_stores_inf(cuda, up):
    """A gradient is stored IEEE: where the true gx exceeds the f16 range the (f16, f16, f16) instance stores inf of
    its sign for the loss scaler to see, never the saturated 65504."""
    gid, _, pad, h, w = REAL_GEO[up]
    fu, fd = sc.r256_filters(up)
    x, gout, _, _ = sc.case_inputs(gid, up, pad, h, w, "linear", F16, F16)
    gout = torch.where(gout != 0, torch.full_like(gout, 60000.0), gout)
    gout[..., 1] = -gout[..., 1]
    rc, got, _ = run_bwd(cuda, x, gout, F16, fu, fd, up, pad, 1.0, -1.0, 0, want_ydot=False)
    assert rc == 0, nv.load().ic2_last_error().decode()
    r = fo.reference(x, gout, fu, fd, up, pad, slope=1.0, clamp=-1.0, eps_x=sc.EPS_X, c=C)
    over = r["ref"].abs() > 65520.0 * (1 + 2.0 ** -10)     # past the f16 overflow threshold with the rounding bound to spare
    under = r["ref"].abs() < 65000.0
    g = got.double()[..., :C]
    assert over.any() and (over & (r["ref"] < 0)).any() and under.any()
    assert torch.isinf(g[over]).all() and (torch.sign(g[over]) == torch.sign(r["ref"][over])).all()
    assert torch.isfinite(g[under]).all() and not torch.isnan(g).any()
    assert not (g.abs() == 65504.0)[over].any()


@pytest.mark.parametrize("what", ["fd_taps_11", "up_3", "out_size"])
def test_kernel_refusals_write_nothing(cuda, what):
    gid, up, pad, h, w = REAL_GEO[2]
    fu, fd = sc.nonsym_filters(2)
    x, gout, os_, b = sc.case_inputs(gid, up, pad, h, w, "mask")
    kw, code = {}, UNSUPPORTED
    if what == "fd_taps_11":
        kw["fd_taps"] = 11
    elif what == "up_3":
        up, fu = 3, torch.cat([fu, fu[:6]])
    else:
        kw["out_hw"], code = (gout.shape[1] + 1, gout.shape[2]), INVALID
    rc, got, yd = run_bwd(cuda, x, gout, F32, fu, fd, up, pad, 0.2, 256.0, 0, os_, b, **kw)
    assert rc == code, (rc, nv.load().ic2_last_error().decode())
    assert torch.isnan(got).all() and torch.isnan(yd).all()


# ------------------------------------------------------------------ fused vs composed
@pytest.mark.parametrize("up", [2, 4])
def test_fused_agrees_with_the_composed_fallback(cuda, up):
    """autograd_ops._flrelu_backward_composed (the fallback on IC2_E_UNSUPPORTED: sg3_ops.filtered_lrelu_backward
    through ic2_upfirdn2d) handles a 2-D down filter and agrees with the fused kernel within the kernel test's own
    bound: |fused - composed| <= K_BAR eps B + eps_out |ref| + A.  The composed path's own error against the reference
    is printed, not gated (it is not the code under test here)."""
    geo = REAL_GEO[up]
    gid, _, pad, h, w = geo
    fu, fd = sc.nonsym_filters(up)
    x, gout, _, _ = sc.case_inputs(gid, up, pad, h, w, "mask")
    rc, fused, _ = run_bwd(cuda, x, gout, F32, fu, fd, up, pad, 0.2, 256.0, 0, want_ydot=False)
    assert rc == 0, nv.load().ic2_last_error().decode()
    L = types.SimpleNamespace(out_channels=C, up_factor=up, down_factor=2, padding=list(pad), up_taps=6 * up,
                              conv_clamp=256.0, act_gain=float(fo.GAIN), up_filter=fu.to(cuda), down_filter=fd.to(cuda))
    comp = ao._flrelu_backward_composed(x.to(cuda), gout.to(cuda), L).cpu()
    r = sc.reference((gid, "nonsym", "mask", 0, F32, F32, False, False), x, gout, fu, fd, up, pad, "mask", 0, None, None)
    d = (fused.double() - comp.double())[..., :C].abs()
    bound = K_BAR * EPS * r["B"] + EPS_OUT[F32] * r["ref"].abs() + r["A"]
    assert (comp[..., C:] == 0).all() and comp.abs().max() > 0
    clean = (r["A"] == 0) & (r["B"] > 0)
    ec = (comp.double()[..., :C] - r["ref"]).abs()
    print(f"[sg3r-bwd] {gid} fused vs composed: max |d| {d.max().item():.3e}, worst d/bound "
          f"{(d / bound.clamp_min(1e-300)).max().item():.3f}, max d/(eps B) {(d[clean] / (EPS * r['B'][clean])).max().item():.3f}; "
          f"composed vs reference max err/(eps B) {(ec[clean] / (EPS * r['B'][clean])).max().item():.3f}")
    assert (d[r["B"] == 0] == 0).all()
    assert (d <= bound).all()


# ------------------------------------------------------------------ FilteredLReluNHWC on a radial layer
@pytest.mark.parametrize("li", [1, 2])
def test_filtered_lrelu_function_radial_layer_fp32(cuda, li):
    """autograd_ops.FilteredLReluNHWC applied to a radial layer (L1: up 2, L2: up 4 of the WIDE R generator) in fp32:
    its backward takes ic2_flrelu_bwd_nhwc_2d's (f32, f32, f32) instance with oscale, bias and ydot NULL.  Forward and
    gradient against autograd through the oracle's filtered_lrelu in fp64 with the layer's 2-D down filter; bound and
    input as test_gpu_training.py::test_flrelu_backward_kernel (clamp reached on a third of the channels)."""
    G, _, _ = _gen(cuda, "wide", True)
    L = G.synthesis.layers()[li]
    assert L.down_radial and L._fd.shape == (12, 12) and L.up_factor == {1: 2, 2: 4}[li]
    c, cp = L.out_channels, L.cout_p
    s = int(L.in_size[0]) + L.conv_kernel - 1
    g = torch.Generator().manual_seed(60 + li)
    y = torch.randn(2, s, s, c, generator=g) * 3
    y[..., : c // 3] = y[..., : c // 3] * 60 + 150
    y = F.pad(y, (0, cp - c))
    yd = y.to(cuda).requires_grad_(True)
    calls = []
    lib = nv.load()

    class _Lib:   # records the 2-D entry point's return codes, forwards everything else to the library
        def __getattr__(self, name):
            return getattr(lib, name)

        def ic2_flrelu_bwd_nhwc_2d(self, *a):
            calls.append(lib.ic2_flrelu_bwd_nhwc_2d(*a))
            return calls[-1]

    out = ao.FilteredLReluNHWC.apply(yd, L, torch.float32)
    gout = F.pad(torch.randn(out.shape[:3] + (c,), generator=g), (0, cp - c))
    nv._lib = _Lib()
    try:
        out.backward(gout.to(cuda))
    finally:
        nv._lib = lib
    assert calls == [0], "the backward must run the fused 2-D kernel, not the composed fallback"
    yr = y.double()[..., :c].permute(0, 3, 1, 2).requires_grad_(True)
    o = sg3.filtered_lrelu(yr, L.up_filter.double().cpu(), L.down_filter.double().cpu(), up=L.up_factor, down=L.down_factor,
                           padding=L.padding, clamp=256)
    o.backward(gout.double()[..., :c].permute(0, 3, 1, 2))
    got = yd.grad.cpu()
    assert got.dtype == torch.float32 and (c == cp or got[..., c:].abs().max().item() == 0.0)
    ef = _rel(out[..., :c].permute(0, 3, 1, 2), o)
    e = _rel(got[..., :c].permute(0, 3, 1, 2), yr.grad)
    print(f"[sg3r-train] FilteredLReluNHWC L{li} fp32: rel error out {ef:.2e}, grad {e:.2e}")
    assert ef < 1e-5 and e < 1e-3


# ------------------------------------------------------------------ the wide input modulation's backward
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("cp", [640, 1024])
def test_scale_bwd_past_512_channels(cuda, cp, dtype):
    """ic2_scale_bwd_nhwc at R's channel counts (a thread walks several channel pairs past 512): dx = da * xscale and
    d xscale = sum_p da * x against fp64 on the stored operands; products are exact in f32, so the sums carry the f32
    accumulation of hw terms and dx one output rounding.  Fails on the parent commit, which refused c_p > 512."""
    n, hw = 2, 37 * 5
    g = torch.Generator().manual_seed(cp)
    da = torch.randn(n, hw, cp, generator=g).to(dtype)
    x = torch.randn(n, hw, cp, generator=g).to(dtype)
    xs = torch.randn(n, cp, generator=g)
    dad, xd, xsd = da.to(cuda), x.to(cuda), xs.to(cuda)
    npart = int(nv.query("ic2_scale_bwd_part_floats", n, hw, cp))
    pbase, part = _guarded([npart], F32, cuda)
    dbase, dx = _guarded([n, hw, cp], dtype, cuda)
    nv.call("ic2_scale_bwd_nhwc", nv.ptr(dad), nv.ptr(xd), nv.ptr(xsd), nv.ptr(dx), nv.dtype_code(dtype), n, hw, cp,
            nv.ptr(part), npart, nv.stream_of(xd))
    torch.cuda.synchronize()
    assert _guards_intact(pbase, npart) and _guards_intact(dbase, dx.numel())
    rdx = da.double() * xs.double()[:, None, :]
    rs = (da.double() * x.double()).sum(1)
    ra = (da.double() * x.double()).abs().sum(1)
    got = part.cpu().double().view(n, -1, cp).sum(1)
    assert torch.isfinite(part).all() and torch.isfinite(dx.float()).all()
    tiny = 2.0 ** -25 if dtype == F16 else 0.0     # an f16 dx below 2^-14 rounds to the subnormal spacing 2^-24
    assert ((dx.cpu().double() - rdx).abs() <= (EPS_OUT[dtype] + 2 * EPS) * rdx.abs() + tiny).all()
    assert ((got - rs).abs() <= (hw + 2) * EPS * ra).all()


# ------------------------------------------------------------------ generators
SMALL = dict(z_dim=32, w_dim=32, img_resolution=32, num_layers=6, channel_base=256, channel_max=24)
WIDE = dict(z_dim=64, w_dim=64, img_resolution=32, num_layers=6, channel_base=2560, channel_max=640)
_gens = {}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _table_kw(cfg, conv_kernel):
    return dict(num_layers=cfg["num_layers"], channel_base=cfg["channel_base"], channel_max=cfg["channel_max"],
                conv_kernel=conv_kernel)


def _gen(cuda, cfg_name, radial):
    """(generator on the device, fp32 state dict for the oracle, layer-table kwargs): built once."""
    key = (cfg_name, radial)
    if key not in _gens:
        cfg = dict(SMALL if cfg_name == "small" else WIDE)
        torch.manual_seed(21)
        kw = dict(conv_kernel=1, use_radial_filters=True) if radial else {}
        G = ic2.Generator(**cfg, **kw).eval().requires_grad_(False)
        with torch.no_grad():  # non-unit input gains, as in a trained generator
            for i, L in enumerate(G.synthesis.layers()):
                L.magnitude_ema.fill_(0.6 + 0.05 * i)
        sd = {k: v.detach().float().cpu() for k, v in G.state_dict().items()}
        tkw = _table_kw(cfg, 1 if radial else 3)
        if radial:
            so.patch_state_dict(sd, cfg["img_resolution"], **tkw)
        _gens[key] = (G.to(cuda), sd, tkw)
    return _gens[key]


# ------------------------------------------------------------------ layer
def _layer_case(cuda, radial, li, bf16):
    """Relative errors (d/dx, d/dw) of layer `li` of the WIDE generator against autograd through the fp64 oracle."""
    G, sd, tkw = _gen(cuda, "wide", radial)
    if radial:
        G.set_radial_training()
    _, table = sg3.layer_table(32, **tkw)
    spec = table[li]
    layer = G.synthesis.layers()[li]
    assert layer.down_radial == radial and G.synthesis.layer_names[li] == spec["name"]
    g = torch.Generator().manual_seed(20 + li)
    x = torch.randn(2, spec["in_channels"], spec["in_size"], spec["in_size"], generator=g)
    w = torch.randn(2, 64, generator=g)
    try:
        if bf16:
            x = x.to(BF16).float()
            xn = F.pad(x.permute(0, 2, 3, 1), (0, layer.cin_p - spec["in_channels"])).to(cuda, BF16)
            xd, wd = xn.requires_grad_(True), w.to(cuda).requires_grad_(True)
            y = layer.forward_train_nhwc(xd, wd, BF16)[..., : spec["out_channels"]].permute(0, 3, 1, 2)
        else:
            xd, wd = x.to(cuda).requires_grad_(True), w.to(cuda).requires_grad_(True)
            y = layer(xd, wd)
        r = torch.randn(y.shape, generator=g)
        (y.float() * r.to(cuda)).sum().backward()
    finally:
        G.set_radial_training(False)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = sg3.synthesis_layer(sd, spec, xr, wr, dtype=torch.float64)
    (yr * r.double()).sum().backward()
    gx = xd.grad[..., : spec["in_channels"]].permute(0, 3, 1, 2) if bf16 else xd.grad
    return _rel(y, yr), _rel(gx, xr.grad), _rel(wd.grad, wr.grad), layer


@pytest.mark.parametrize("li", [1, 2])
def test_layer_gradients_fp32(cuda, li):
    """SynthesisLayer(x, w) of an R layer with grad (L1: 640 -> 384 channels at 36^2, up 2; L2: 384 -> 256, 36 -> 52, up
    4): d/dx and d/dw against autograd through the fp64 oracle layer on the patched state dict.  1e-3: the T test's
    bound (test_gpu_training.py::test_synthesis_layer_gradients_fp32) with the same lrelu-side argument."""
    ey, ex, ew, layer = _layer_case(cuda, True, li, False)
    assert layer.conv_kernel == 1 and (layer.cin_p, layer.cout_p) == {1: (640, 384), 2: (384, 256)}[li]   # padded
    assert layer.up_factor == {1: 2, 2: 4}[li] and int(layer.in_size[0]) == 36
    print(f"[sg3r-train] layer {li} fp32: rel error y {ey:.2e}, grad x {ex:.2e}, grad w {ew:.2e}")
    assert ex < 1e-3 and ew < 1e-3


# (x, w) relative gradient error bounds of the bf16 R layer test: 3x the MI355X measurement (see the docstring)
_BF16_LAYER_TOL = {1: (0.024, 0.024), 2: (0.020, 0.022)}


@pytest.mark.parametrize("li", [1, 2])
def test_layer_gradients_bf16_beside_t(cuda, li):
    """The bf16 training step of one R layer (forward_train_nhwc) against the fp64 oracle on the same bf16-rounded
    input, with the T layer of the same shape (conv_kernel 3, separable filters: existing code) beside it.  Bound: 3x
    the error measured on MI355X, and R within 2x of T.  Measured (profiles/r17_sg3r_train.txt), x / w: L1 R 8.08e-3 /
    8.01e-3, T 8.75e-3 / 8.03e-3; L2 R 6.88e-3 / 7.47e-3, T 7.14e-3 / 6.61e-3."""
    ey, ex, ew, _ = _layer_case(cuda, True, li, True)
    ty_, tx_, tw_, _ = _layer_case(cuda, False, li, True)
    print(f"[sg3r-train] layer {li} bf16: R rel error y {ey:.2e}, grad x {ex:.2e}, grad w {ew:.2e}; "
          f"T y {ty_:.2e}, grad x {tx_:.2e}, grad w {tw_:.2e}")
    bx, bw = _BF16_LAYER_TOL[li]
    assert ex < bx and ew < bw
    assert ex <= 2 * tx_ and ew <= 2 * tw_


# ------------------------------------------------------------------ network
_net = {}


def _net_case(cuda, radial):
    """(G, ws, cotangent r, fp64 oracle dL/dws): the oracle gradient is computed once per module."""
    if radial not in _net:
        G, sd, tkw = _gen(cuda, "small", radial)
        ws = torch.randn(2, G.num_ws, G.w_dim, generator=torch.Generator().manual_seed(3)) * 0.7
        r = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(6))
        wr = ws.double().requires_grad_(True)
        img = sg3.synthesis_forward(sd, 32, wr, dtype=torch.float64, **tkw)
        (img * r.double()).sum().backward()
        _net[radial] = (G, ws, r, wr.grad.detach())
    return _net[radial]


def _net_err(cuda, radial, precision):
    G, ws, r, ref = _net_case(cuda, radial)
    scale = 4096.0 if precision == "f16" else 1.0     # f16: the loss scaled by 2^12 as a GradScaler would
    G.set_precision(precision)
    G.synthesis.train_f16 = precision == "f16"
    G.set_radial_training(radial)
    try:
        with torch.no_grad():
            inf = G.synthesis(ws.to(cuda))
        wd = ws.to(cuda).requires_grad_(True)
        img = G.synthesis(wd)
        assert img.grad_fn is not None and img.shape == (2, 3, 32, 32)
        d_fwd = (img.detach() - inf).abs().max().item()
        (img * r.to(cuda) * scale).sum().backward()
        grad = wd.grad / scale
    finally:
        G.set_precision("fp32")
        G.synthesis.train_f16 = False
        G.set_radial_training(False)
    assert torch.isfinite(grad).all()
    return _rel(grad, ref), d_fwd


@pytest.mark.parametrize("precision", ["fp32", "bf16", "f16"])
def test_network_gradient_wrt_ws(cuda, precision):
    """dL/dws through the whole frozen SMALL R synthesis against autograd through the fp64 oracle, beside the T
    generator of the same small shape (conv_kernel 3, separable filters: existing code).  fp32 < 1e-3; bf16 and f16
    (train_f16, loss x 2^12): at most 2x T's error measured in the same test.  The autograd forward equals the
    no-grad forward within the T test's limits.  Measured: profiles/r17_sg3r_train.txt."""
    e_r, d_r = _net_err(cuda, True, precision)
    e_t, d_t = _net_err(cuda, False, precision)
    print(f"[sg3r-train] network {precision}: rel grad error R {e_r:.3e}  T {e_t:.3e}; "
          f"|train fwd - inference fwd| R {d_r:.2e}  T {d_t:.2e}")
    assert d_r < {"fp32": 1e-4, "bf16": 2e-2, "f16": 4e-3}[precision]
    if precision == "fp32":
        assert e_r < 1e-3
    else:
        assert e_r <= 2 * e_t


# ------------------------------------------------------------------ step
def _compressor(cuda, G):
    torch.manual_seed(7)
    enc = ic2.HVAE_VGG_Encoder(img_resolution=64, w_dim=G.w_dim, num_ws=G.num_ws, block_split=(3, 6), channel_base=256,
                               channel_max=32, fix_fine_projector=True).to(cuda)
    return enc, ic2.StyleGAN3Compressor(enc, G, training_resolution=64)


def test_train_step_through_r_generator(cuda):
    G, _, _ = _gen(cuda, "small", True)
    enc, comp = _compressor(cuda, G)
    opt = ict.make_optimizer(enc, lr=1e-3)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    w_avg = G.mapping.w_avg.view(1, 1, -1)
    G.set_radial_training()
    try:
        torch.manual_seed(3)
        out0 = ict.train_step(comp, x, opt, w_avg, perceptual_weight=0.0)
        grads = {k: v.grad.detach().clone() for k, v in enc.named_parameters()}
        torch.manual_seed(3)
        out1 = ict.train_step(comp, x, opt, w_avg, perceptual_weight=0.0)
    finally:
        G.set_radial_training(False)
    v0, v1 = ({k: v.item() for k, v in o.items()} for o in (out0, out1))
    assert all(np.isfinite(v) for v in list(v0.values()) + list(v1.values())), (v0, v1)
    for k, g in grads.items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
    assert v0["total_loss"] != v1["total_loss"] and v0["rec_loss"] != v1["rec_loss"]
    assert all(p.grad is None for p in G.parameters())


def test_train_step_f16_scaler_skips_an_overflow(cuda):
    """make_f16 + train_step(scaler=...) on the R generator: a clean step keeps the scale and moves the encoder; an
    injected overflow (an image scale far outside the f16 range of the reconstruction gradient) skips the step and
    backs the scale off."""
    G, _, _ = _gen(cuda, "small", True)
    enc, comp = _compressor(cuda, G)
    opt = ict.make_optimizer(enc, lr=1e-4)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    w_avg = G.mapping.w_avg.view(1, 1, -1)
    scaler = ict.make_f16(comp)
    G.set_radial_training()
    try:
        before = {k: v.detach().clone() for k, v in enc.named_parameters()}
        out = ict.train_step(comp, x, opt, w_avg, perceptual_weight=0.0, scaler=scaler)
        assert all(np.isfinite(v.item()) for v in out.values())
        assert scaler.get_scale() == 65536.0
        changed = [k for k, v in enc.named_parameters() if not torch.equal(v.detach(), before[k])]
        assert len(changed) >= len(before) // 2, changed
        snap = {k: v.detach().clone() for k, v in enc.named_parameters()}
        ict.train_step(comp, x * 1e30, opt, w_avg, perceptual_weight=0.0, scaler=scaler)
        assert scaler.get_scale() == 32768.0
        assert all(torch.equal(v.detach(), snap[k]) for k, v in enc.named_parameters())
    finally:
        G.set_precision("fp32")
        G.synthesis.train_f16 = False
        G.set_radial_training(False)


# ------------------------------------------------------------------ switch
def test_without_the_switch_every_entry_refuses(cuda):
    G, _, _ = _gen(cuda, "small", True)
    assert G.synthesis.train_radial is False
    ws = torch.randn(2, G.num_ws, G.w_dim, device=cuda, requires_grad=True)
    with pytest.raises(nv.AutogradUnsupported, match="StyleGAN3-R"):
        G.synthesis(ws)
    L = G.synthesis.layers()[1]
    x = torch.randn(2, L.in_channels, 36, 36, device=cuda, requires_grad=True)
    with pytest.raises(nv.AutogradUnsupported, match="StyleGAN3-R"):
        L(x, torch.randn(2, G.w_dim, device=cuda))
    enc, comp = _compressor(cuda, G)
    opt = ict.make_optimizer(enc)
    img = (torch.rand(2, 3, 64, 64, device=cuda) * 2 - 1)
    with pytest.raises(nv.AutogradUnsupported, match="StyleGAN3-R"):
        ict.train_step(comp, img, opt, G.mapping.w_avg.view(1, 1, -1), perceptual_weight=0.0)
    # the no-grad forward is the same with the switch set
    with torch.no_grad():
        a = G.synthesis(ws.detach())
        G.set_radial_training()
        b = G.synthesis(ws.detach())
        G.set_radial_training(False)
    assert torch.equal(a, b)


def test_zz_report_measured_ratios():
    """Prints the largest |got - ref| / (eps B) each tier reached over the f32-output cases above (the `measured` of
    the module docstring); the bar must not exceed the derived count."""
    for tier, v in sorted(RATIOS.items()):
        print(f"[sg3r-bwd measured] {tier}: max err/(eps B) {v:.3f}, bar {K_BAR}, derived {K_DERIVED}")
    assert K_BAR <= K_DERIVED
