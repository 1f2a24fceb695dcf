"""The filtered-lrelu backward kernels (csrc/flrelu_bwd.hip: VALU, 16x16 gx tiles; csrc/flrelu_bwd_mfma.hip: the
persistent strip kernel, 16-row tiles, 16- / 8-column strips) per element at edge geometries, against the fp64
reference of tests/flrelu_bwd_oracle.py (pinned by tests/test_flrelu_bwd_oracle_host.py), and a few forward cases
with the same asymmetric taps.  Every backward call goes through the C ABI (ic2_flrelu_bwd_nhwc_ex) with gx and ydot
NaN-prefilled between sentinel guard bands.

Two tiers per geometry, both per element with B (magnitude bound) and A (mask allowance) from the oracle:

  linear  slope 1, no clamp: |got - ref| <= K eps B + eps_out |ref|
  mask    slope 0.2, clamp 256 on block-sign inputs: |got - ref| <= K eps B + eps_out |ref| + A, and A > 0 on at most
          20 % of the elements (asserted on the reference alone, here and in the host test)

eps is the unit of the gradient arithmetic as the paths' tests count it: 2^-9 (bf16 operands), 2^-12 (f16 operands),
2^-24 (the VALU kernel, f32 arithmetic on exactly representable operands whatever their storage dtype); eps_out the
unit roundoff of the stored gx (2^-8 bf16, 2^-11 f16, 2^-24 f32).

K per path: derived count of roundings / measured max |got - ref| / (eps B) over all cases of this file / bar.
The bar is at most min(derived, 2 x measured); the figures are recorded in profiles/r15_flr_bwd_edges.txt:

  mfma, bf16 gradients  derived 16: the four tap matrices in bf16 (gd vertical, gd horizontal, gu^T horizontal, gu^T
                        vertical) and the three stored intermediates (GAv, GU, P), 7 roundings of 2^-8 = 2 eps each,
                        plus the taps' joint f16 rounding (either neighbour: 2^-10 = eps / 2) in the four passes.
                        Measured 7.31 (linear), 7.08 (mask), both at the one-column crop u2-crop11_12-33x23, where B is
                        close to |ref| and 2 of the 7.3 are the output rounding; bar 9.
  mfma, f16 gradients   derived 22: the same three intermediates in f16 (2^-11 = 2 eps each) and the f16 taps of the
                        four passes (2^-10 = 4 eps each).  Measured 1.77 (linear), 2.06 (mask); bar 3.5.
  valu                  derived 26: f32 FMA chains of 6 taps in each of the four passes, the activation product and the
                        oscale product.  Measured 3.37 (linear), 3.24 (mask) over the f32-output instances (the bf16
                        output's own rounding, eps_out, is 2^16 eps and is left out of the measure there); bar 6.
"""
import ctypes

import numpy as np
import pytest
import torch

import flrelu_bwd_oracle as fo
from image_compression_2_amd import _native as nv
from oracle import sg3

pytestmark = pytest.mark.gpu

GUARD = 8192
SENTINEL = -1536.0  # exact in f16, bf16 and f32
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EPS = {BF16: 2.0 ** -9, F16: 2.0 ** -12, F32: 2.0 ** -24}
EPS_OUT = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}
# derived count, bar (see the module docstring)
K_DERIVED = {"mfma_bf16": 16.0, "mfma_f16": 22.0, "valu": 26.0}
K_BAR = {"mfma_bf16": 9.0, "mfma_f16": 3.5, "valu": 6.0}
INVALID, UNSUPPORTED = 1, 2


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


def _path_of(xdt, gdt, odt):
    if xdt == F16 and ((gdt == BF16 and odt == BF16) or gdt == F16):
        return "mfma_f16" if gdt == F16 else "mfma_bf16"
    return "valu"


def run_bwd(dev, x, gout, odt, fu, fd, up, pad, slope, clamp, flip, oscale=None, bias=None, want_ydot=True,
            out_hw=None, ydot_short=0, taps=None, down=2, legacy=False):
    """One call of ic2_flrelu_bwd_nhwc_ex (legacy: ic2_flrelu_bwd_nhwc) -> (rc, gx on the host, ydot on the host or
    None).  gx and ydot are NaN-prefilled between guard bands; the guards are asserted intact."""
    n, h, w, cp = x.shape
    oh, ow = gout.shape[1:3] if out_hw is None else out_hw
    xd, gd = x.to(dev), gout.to(dev)
    osd = None if oscale is None else oscale.to(dev)
    bd = None if bias is None else bias.to(dev)
    gbase, gx = _guarded([n, h, w, cp], odt, dev)
    nyd = int(nv.query("ic2_flrelu_bwd_ydot_floats", n, cp, h, w, up))
    assert nyd == n * -(-h // 16) * -(-w // 16) * cp
    ybase, yd = _guarded([nyd], F32, dev) if want_ydot else (None, None)
    fua, fup = _fp(fu)
    fda, fdp = _fp(fd)
    tu, td = taps if taps is not None else (fua.shape[0], fda.shape[0])
    lib = nv.load()
    if legacy:
        assert odt == F32 and oscale is None and bias is None and not want_ydot
        rc = lib.ic2_flrelu_bwd_nhwc(nv.ptr(xd), nv.dtype_code(x.dtype), nv.ptr(gd), nv.dtype_code(gout.dtype), nv.ptr(gx),
                                     n, cp, h, w, oh, ow, fup, tu, fdp, td, up, down, *pad, float(fo.GAIN), slope, clamp,
                                     int(flip), nv.stream_of(xd))
    else:
        rc = lib.ic2_flrelu_bwd_nhwc_ex(nv.ptr(xd), nv.dtype_code(x.dtype), nv.ptr(gd), nv.dtype_code(gout.dtype),
                                        nv.ptr(gx), nv.dtype_code(odt), n, cp, h, w, oh, ow, fup, tu, fdp, td, up, down,
                                        *pad, float(fo.GAIN), slope, clamp, int(flip), nv.ptr(osd), nv.ptr(bd),
                                        nv.ptr(yd), nyd - ydot_short if want_ydot else 0, nv.stream_of(xd))
    torch.cuda.synchronize()
    assert _guards_intact(gbase, gx.numel()), "store outside gx"
    if want_ydot:
        assert _guards_intact(ybase, nyd), "store outside ydot"
    return rc, gx.cpu(), (yd.cpu() if want_ydot else None)


RATIOS = {}


def check_gx(got, r, key, odt, gdt, tier, c, tag):
    """The per-element bound of the module docstring; prints the measured ratio, then asserts."""
    g = got.double()
    assert torch.isfinite(g).all(), f"{tag}: gx not written everywhere"
    assert (g[..., c:] == 0).all(), f"{tag}: padded channels of gx"
    eps = EPS[F32] if key == "valu" else EPS[gdt]
    err = (g[..., :c] - r["ref"]).abs()
    lin = K_BAR[key] * eps * r["B"] + EPS_OUT[odt] * r["ref"].abs()
    bound = lin + (r["A"] if tier == "mask" else 0.0)
    # measured: the rounding share of the error over eps B, where no mask decision can differ
    clean = (r["A"] == 0) & (r["B"] > 0)
    ratio = ((err - EPS_OUT[odt] * r["ref"].abs()).clamp_min(0)[clean] / (eps * r["B"][clean])).max().item()
    raw = (err[clean] / (eps * r["B"][clean])).max().item()
    RATIOS[key, tier] = max(RATIOS.get((key, tier), 0.0), raw if EPS_OUT[odt] <= 2 * eps else ratio)
    share = (r["A"] > 0).double().mean().item()
    bad = err > bound
    print(f"[flrelu-bwd-edges] {tag} {key} {tier}: max err/(eps B) {raw:.3f} (less the output rounding {ratio:.3f}), "
          f"A > 0 on {100 * share:.1f} %, over the bound {int(bad.sum())} of {bad.numel()}"
          + (f", worst err/bound {(err / bound.clamp_min(1e-300))[bad].max().item():.2f}" if bad.any() else ""))
    if tier == "mask":
        assert share <= 0.20, f"{tag}: mask allowance on {100 * share:.1f} % of the elements"
    else:
        assert r["A"].abs().max().item() == 0.0
    assert (r["B"] > 0).any()
    assert not bad.any(), f"{tag}: {int(bad.sum())} elements over the bound, first at {bad.nonzero()[0].tolist()}"


def check_ydot_valu(yd, r, key, tier, c, tag):
    """ydot [n][tile][c_p] of the VALU kernel: every 16x16 tile's partial (partial tiles included) against the reference
    restricted to that tile.  Bound: the gx bound (unscaled) times |x - bias| summed over the tile, plus the f32
    accumulation of up to 256 products (2^-24 each, 258 roundings at the most) on the sum of magnitudes."""
    n, h, w, _ = r["ref0"].shape
    ty, tx = -(-h // 16), -(-w // 16)
    y = yd.view(n, ty * tx, -1).double()
    assert torch.isfinite(y).all() and (y[..., c:] == 0).all(), tag
    xb = r["x"] - r["bias"]
    per = K_BAR[key] * EPS[F32] * r["B0"] + (r["A0"] if tier == "mask" else 0.0)
    worst = 0.0
    for j in range(ty):
        for i in range(tx):
            sl = (slice(None), slice(16 * j, 16 * j + 16), slice(16 * i, 16 * i + 16))
            ref = (r["ref0"][sl] * xb[sl]).sum(dim=(1, 2))
            tol = (per[sl] * xb[sl].abs()).sum(dim=(1, 2)) + 258 * 2.0 ** -24 * (r["ref0"][sl] * xb[sl]).abs().sum(dim=(1, 2))
            e = (y[:, j * tx + i, :c] - ref).abs()
            worst = max(worst, (e / tol.clamp_min(1e-300)).max().item())
            assert (e <= tol).all(), f"{tag}: ydot of tile ({j}, {i}) off by {(e / tol.clamp_min(1e-300)).max().item():.2f} bounds"
    print(f"[flrelu-bwd-edges] {tag} valu ydot: {ty * tx} tiles, worst err/bound {worst:.3f}")


def check_ydot_mfma(yd, got, r, key, odt, gdt, tier, c, tag):
    """ydot [n][chunk][c_p] of the MFMA path: chunk k covers the pixels [k per, (k + 1) per) of the flattened image, per =
    ceil(h w / chunks) (flrelu_bwd_mfma_launch), and holds sum stored gx * (x - bias) / oscale (0 where oscale is 0) --
    from the STORED gx, as the kernel documents.  Bound per chunk: the f32 accumulation of `per` products.  The chunk
    sum is also compared with the true sum (dL/dx) (x - bias) at the gx bound."""
    n, h, w, _ = r["ref0"].shape
    hw, nch = h * w, -(-h // 16) * -(-w // 16)
    per = -(-hw // nch)
    y = yd.view(n, nch, -1).double()
    assert torch.isfinite(y).all() and (y[..., c:] == 0).all(), tag
    osb = r["os"][:, None, :]                                    # [n, 1, c]
    live = osb != 0
    xb = (r["x"] - r["bias"]).reshape(n, hw, c)
    term = got.double()[..., :c].reshape(n, hw, c) * xb / torch.where(live, osb, torch.ones_like(osb))
    term = torch.where(live, term, torch.zeros_like(term))
    worst = 0.0
    for k in range(nch):
        sl = slice(min(k * per, hw), min((k + 1) * per, hw))
        ref = term[:, sl].sum(1)
        tol = (per + 16) * 2.0 ** -24 * term[:, sl].abs().sum(1)
        e = (y[:, k, :c] - ref).abs()
        worst = max(worst, (e / tol.clamp_min(1e-300)).max().item())
        assert (e <= tol).all(), f"{tag}: ydot of chunk {k} off by {(e / tol.clamp_min(1e-300)).max().item():.2f} bounds"
    assert (y[:, :, :c][~live.expand(n, nch, c)] == 0).all(), f"{tag}: ydot where oscale is 0"
    per_el = K_BAR[key] * EPS[gdt] * r["B0"] + EPS_OUT[odt] * r["ref0"].abs() + (r["A0"] if tier == "mask" else 0.0)
    tol = (per_el.reshape(n, hw, c) * xb.abs()).sum(1) + 2.0 ** -20 * (r["ref0"].reshape(n, hw, c) * xb).abs().sum(1)
    true = torch.where(live[:, 0], r["ydot"], torch.zeros_like(r["ydot"]))
    e = (y[:, :, :c].sum(1) - true).abs()
    assert (e <= tol).all(), f"{tag}: chunk sum of ydot off by {(e / tol.clamp_min(1e-300)).max().item():.2f} bounds"
    print(f"[flrelu-bwd-edges] {tag} mfma ydot: {nch} chunks of {per}, worst err/bound {worst:.3f}, "
          f"sum err/bound {(e / tol.clamp_min(1e-300)).max().item():.3f}")


def run_case(dev, tag, x, gout, odt, up, pad, tier, flip, oscale, bias, want_ydot=True, asym=True, c=fo.C):
    """Run one call and check gx (and ydot) against the reference of the same stored operands."""
    fu, fd = fo.taps(up, asym)
    kw = fo.TIERS[tier]
    key = _path_of(x.dtype, gout.dtype, odt)
    rc, got, yd = run_bwd(dev, x, gout, odt, fu, fd, up, pad, kw["slope"], kw["clamp"], flip, oscale, bias, want_ydot)
    assert rc == 0, nv.load().ic2_last_error().decode()
    r = fo.reference(x, gout, fu, fd, up, pad, flip=bool(flip), oscale=oscale, bias=bias,
                     eps_x=fo.EPS_X["valu" if key == "valu" else "mfma"], c=c, **kw)
    check_gx(got, r, key, odt, gout.dtype, tier, c, tag)
    if want_ydot:
        if key == "valu":
            check_ydot_valu(yd, r, key, tier, c, tag)
        else:
            check_ydot_mfma(yd, got, r, key, odt, gout.dtype, tier, c, tag)
    return got, yd, r


GEOS = fo.geometries()


# ------------------------------------------------------------------ the edge sweep
@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("geo", GEOS, ids=[g[0] for g in GEOS])
def test_flrelu_bwd_edge_geometry(cuda, geo, path):
    """Every geometry of the sweep on both paths (mfma: f16 x, bf16 gout and gx; valu: f32 throughout), both tiers,
    flip 0 and 1, asymmetric taps, oscale, bias and ydot set, two samples with different data."""
    gid, up, pad, h, w = geo
    odt = BF16 if path == "mfma" else F32
    for tier in ("linear", "mask"):
        x, gout, os_, b = fo.case_inputs(gid, up, pad, h, w, path, tier)
        for flip in (0, 1):
            run_case(cuda, f"{gid} flip {flip}", x, gout, odt, up, pad, tier, flip, os_, b)


@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("gid", ["u2-p9_8-17x33", "u4-crop6_9-17x21"])
def test_flrelu_bwd_symmetric_taps_and_small_gradients(cuda, gid, path):
    """The symmetric low-pass design of the older tests (flip cannot matter: both flips give the same bits), and the
    mask tier with gout scaled by 1e-7 (below the f16 range on the bf16 path), once per path and up factor."""
    _, up, pad, h, w = [g for g in GEOS if g[0] == gid][0]
    odt = BF16 if path == "mfma" else F32
    x, gout, os_, b = fo.case_inputs(gid, up, pad, h, w, path, "mask")
    g0, y0, _ = run_case(cuda, f"{gid} symmetric", x, gout, odt, up, pad, "mask", 0, os_, b, asym=False)
    g1, y1, _ = run_case(cuda, f"{gid} symmetric flip", x, gout, odt, up, pad, "mask", 1, os_, b, asym=False)
    assert torch.equal(g0, g1) and torch.equal(y0, y1)
    x, gout, os_, b = fo.case_inputs(gid, up, pad, h, w, path, "mask", gscale=1e-7)
    run_case(cuda, f"{gid} gout 1e-7", x, gout, odt, up, pad, "mask", 0, os_, b)


# ------------------------------------------------------------------ dtype and argument matrix
MATRIX_GEO = {2: "u2-p9_8_9_10-17x33", 4: "u4-p15_14-17x9"}
DTYPES = [(F32, F32, F32), (F16, BF16, F32), (F32, BF16, F32), (F16, F32, F32), (F32, F32, BF16), (F16, BF16, BF16),
          (F16, F16, F16)]


def _matrix_inputs(up, tier, xdt, gdt):
    gid = MATRIX_GEO[up]
    _, _, pad, h, w = [g for g in GEOS if g[0] == gid][0]
    x, gout, os_, b = fo.case_inputs(gid, up, pad, h, w, "valu", tier)   # f32 draws, rounded to the stored dtypes
    return gid, pad, x.to(xdt), gout.to(gdt), os_, b


@pytest.mark.parametrize("xdt,gdt,odt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_bwd_dtype_matrix(cuda, up, xdt, gdt, odt):
    """Every instance behind the entry point: VALU (f32,f32->f32), (f16,bf16->f32), (f32,bf16->f32), (f16,f32->f32),
    (f32,f32->bf16); MFMA (f16,bf16->bf16), (f16,f16->f16).  Both tiers, flip 1 in the mask tier."""
    for tier, flip in (("linear", 0), ("mask", 1)):
        gid, pad, x, gout, os_, b = _matrix_inputs(up, tier, xdt, gdt)
        run_case(cuda, f"{gid} flip {flip}", x, gout, odt, up, pad, tier, flip, os_, b)


@pytest.mark.parametrize("null", ["oscale", "bias", "ydot", "all"])
@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_bwd_null_arguments(cuda, up, path, null):
    """oscale, bias and ydot NULL in turn and all together (mask tier): the result is the reference of that call."""
    xdt, gdt, odt = (F16, BF16, BF16) if path == "mfma" else (F32, F32, F32)
    gid, pad, x, gout, os_, b = _matrix_inputs(up, "mask", xdt, gdt)
    run_case(cuda, f"{gid} null {null}", x, gout, odt, up, pad, "mask", 0, None if null in ("oscale", "all") else os_,
             None if null in ("bias", "all") else b, want_ydot=null not in ("ydot", "all"))


@pytest.mark.parametrize("xdt,gdt", [(F32, F32), (F16, BF16)], ids=["f32", "f16_bf16"])
@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_bwd_legacy_entry_equals_ex(cuda, up, xdt, gdt):
    """ic2_flrelu_bwd_nhwc is the _ex call with f32 gx and oscale, bias, ydot NULL, bit for bit."""
    gid, pad, x, gout, _, _ = _matrix_inputs(up, "mask", xdt, gdt)
    fu, fd = fo.taps(up)
    rc0, g0, _ = run_bwd(cuda, x, gout, F32, fu, fd, up, pad, 0.2, 256.0, 1, want_ydot=False)
    rc1, g1, _ = run_bwd(cuda, x, gout, F32, fu, fd, up, pad, 0.2, 256.0, 1, want_ydot=False, legacy=True)
    assert rc0 == 0 and rc1 == 0
    assert torch.isfinite(g0).all() and g0.abs().max() > 0 and torch.equal(g0, g1)


@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_bwd_mfma_ydot_zero_oscale(cuda, up):
    """oscale == 0 on one (sample, channel): gx is 0 there and every ydot chunk of it is exactly 0 (the kernel divides
    the stored-gx sums by oscale and must not produce 0 / 0)."""
    gid, pad, x, gout, os_, b = _matrix_inputs(up, "mask", F16, BF16)
    os_ = os_.clone()
    os_[0, 3] = 0.0
    os_[1, 17] = 0.0
    got, yd, _ = run_case(cuda, f"{gid} oscale 0", x, gout, BF16, up, pad, "mask", 0, os_, b)
    y = yd.view(2, -1, fo.C_P)
    assert (got[0, :, :, 3] == 0).all() and (got[1, :, :, 17] == 0).all()
    assert (y[0, :, 3] == 0).all() and (y[1, :, 17] == 0).all() and y[0, :, 17].abs().max() > 0


# ------------------------------------------------------------------ chained strip segments
@pytest.mark.parametrize("up", [2, 4])
def test_flrelu_bwd_mfma_chained_strips(cuda, up):
    """With at least 8 strips per CU (a 512-thread workgroup is resident at most 4 times per CU) fm_strip_segments
    keeps whole strips, so one workgroup walks the three 16-row tiles of in_h = 33 (ring hand-over, accumulator
    shift, stores in flight across tiles) and then further strips.  Kept cheap by replication: every 16-channel
    block of every sample holds the same data, oscale and bias; all of them must equal block 0 of sample 0 bit for
    bit, and that block is compared with the reference per element."""
    n, cp, c = 4, 512, fo.CHAINED_C
    pad, h, w = fo.CHAINED[up]
    strip = 16 if up == 2 else 8
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert n * -(-w // strip) * (cp // 16) >= 8 * cus
    oh, ow = fo.out_size(h, w, up, pad)
    fu, fd = fo.taps(up)
    for tier in ("linear", "mask"):
        kw = fo.TIERS[tier]
        x1, g1, os1, b1 = fo.chained_inputs(up, tier)
        os_, b = os1.repeat(n, cp // 16), b1.repeat(cp // 16)
        x, gout = x1.repeat(n, 1, 1, cp // 16), g1.repeat(n, 1, 1, cp // 16)
        rc, got, yd = run_bwd(cuda, x, gout, BF16, fu, fd, up, pad, kw["slope"], kw["clamp"], 0, os_, b)
        assert rc == 0, nv.load().ic2_last_error().decode()
        blocks = got.view(n, h, w, cp // 16, 16)
        assert torch.equal(blocks, blocks[:1, :, :, :1].expand_as(blocks)), "replicated blocks differ"
        yb = yd.view(n, -1, cp // 16, 16)
        assert torch.equal(yb, yb[:1, :, :1].expand_as(yb)), "replicated ydot blocks differ"
        r = fo.reference(x1, g1, fu, fd, up, pad, flip=False, oscale=os1, bias=b1, eps_x=fo.EPS_X["mfma"], c=c, **kw)
        tag = f"chained u{up} {h}x{w}"
        check_gx(got[:1, :, :, :16], r, "mfma_bf16", BF16, BF16, tier, c, tag)
        check_ydot_mfma(yd.view(n, -1, cp)[:1, :, :16].contiguous(), got[:1, :, :, :16], r, "mfma_bf16", BF16, BF16, tier,
                        c, tag)


# ------------------------------------------------------------------ the entry point's refusals
@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("what", ["px0_ne_py0", "out_h", "f16_grad_bf16_gx", "f16_grad_f32_x", "taps", "up", "ydot_short"])
def test_flrelu_bwd_refusals_write_nothing(cuda, what, path):
    """Each documented refusal returns its code before any launch: gx and ydot keep their NaN prefill."""
    up, pad, h, w = 2, [9, 8, 9, 8], 17, 9
    xdt, gdt, odt = (F16, BF16, BF16) if path == "mfma" else (F32, F32, F32)
    fu, fd = fo.taps(up)
    kw = dict(taps=None, out_hw=None, ydot_short=0)
    code = INVALID
    if what == "px0_ne_py0":
        pad = [9, 8, 10, 7]   # same out_h: only the px0 == py0 rule objects
    elif what == "f16_grad_bf16_gx":
        xdt, gdt, odt = F16, F16, BF16
    elif what == "f16_grad_f32_x":
        xdt, gdt, odt = F32, F16, F16
    elif what == "taps":
        kw["taps"], code = (8, 12), UNSUPPORTED
    elif what == "up":
        up, code = 3, UNSUPPORTED
        fu = torch.cat([fu, fu[:6]])   # 18 = 6 * up taps
    elif what == "ydot_short":
        kw["ydot_short"] = 1
    tu = kw["taps"][0] if kw["taps"] else fu.numel()
    oh, ow = sg3.filtered_lrelu_out_size(h, w, tu, 12, up, 2, pad)
    if what == "out_h":
        kw["out_hw"] = (oh + 1, ow)
    x = fo.gauss(2, h, w, fo.C, fo.C_P, 1, xdt)
    gout = fo.gauss(2, oh + (what == "out_h"), ow, fo.C, fo.C_P, 2, gdt)
    os_, b = fo.scale_bias(2, fo.C, fo.C_P, 3)
    rc, got, yd = run_bwd(cuda, x, gout, odt, fu, fd, up, pad, 0.2, 256.0, 0, os_, b, **kw)
    assert rc == code, (rc, nv.load().ic2_last_error().decode())
    assert torch.isnan(got.float()).all() and torch.isnan(yd).all()


# ------------------------------------------------------------------ forward: asymmetric taps, both flips
FWD_CASES = [(2, [9, 8, 9, 10], 17, 33), (2, [-11, -12, -11, -12], 31, 25), (4, [15, 14, 15, 14], 17, 9),
             (4, [-6, -9, -6, -9], 16, 21)]


def _fwd_ref(x_nchw, fu, fd, b, up, pad, clamp, flip):
    return sg3.filtered_lrelu(x_nchw.double(), fu.double(), fd.double(), None if b is None else b.double(), up=up,
                              down=2, padding=pad, gain=fo.GAIN, slope=0.2, clamp=clamp, flip_filter=bool(flip))


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("up,pad,h,w", FWD_CASES)
def test_flrelu_fwd_nchw_asymmetric_taps(cuda, up, pad, h, w, dtype, flip):
    """ic2_filtered_lrelu (NCHW) with asymmetric taps, flip 0 and 1, at test_filtered_lrelu_nchw's bars."""
    n, c = 2, 19
    g = torch.Generator().manual_seed(200 + up + flip)
    x = (torch.randn(n, c, h, w, generator=g) * 3).to(dtype)
    b = torch.randn(c, generator=g)
    fu, fd = fo.taps(up)
    oh, ow = fo.out_size(h, w, up, pad)
    xd, bd = x.to(cuda), b.to(cuda)
    out = torch.full((n, c, oh, ow), float("nan"), device=cuda, dtype=dtype)
    fua, fup = _fp(fu)
    fda, fdp = _fp(fd)
    nv.call("ic2_filtered_lrelu", nv.ptr(xd), nv.ptr(out), nv.dtype_code(dtype), n, c, h, w, oh, ow, fup, fu.numel(), fdp,
            12, nv.ptr(bd), up, 2, *pad, float(fo.GAIN), 0.2, 5.0, flip, nv.stream_of(xd))
    torch.cuda.synchronize()
    del fua, fda
    r = _fwd_ref(x, fu, fd, b, up, pad, 5.0, flip)
    y = out.double().cpu()
    assert torch.isfinite(y).all()
    tol = 2e-5 if dtype == F32 else 3e-2
    assert (y - r).abs().max().item() < tol * (1 + r.abs().max().item())


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("up,pad,h,w", FWD_CASES)
def test_flrelu_fwd_nhwc_asymmetric_taps(cuda, up, pad, h, w, flip):
    """ic2_flrelu_nhwc with asymmetric taps and flip 0 / 1: bf16 with a bias (the VALU kernel) at
    test_flrelu_nhwc_bf16_bias's bar; f16 -> bf16 without a bias (the MFMA strip kernel) with a post_scale at
    test_flrelu_nhwc_bf16_matches_oracle's bars; ic2_flrelu_nhwc16 on the blocked copy bit-identical to the latter."""
    n, c_p = 2, 32
    g = torch.Generator().manual_seed(300 + up + flip)
    fu, fd = fo.taps(up)
    fua, fup = _fp(fu)
    fda, fdp = _fp(fd)
    oh, ow = fo.out_size(h, w, up, pad)

    def call(fn, src, in_dt, bias, ps, clamp):
        out = torch.full((n, oh, ow, c_p), float("nan"), device=cuda, dtype=BF16)
        nv.call(fn, nv.ptr(src), nv.ptr(out), nv.dtype_code(in_dt), nv.BF16, n, c_p, h, w, oh, ow, fup, fu.numel(), fdp, 12,
                nv.ptr(bias), up, 2, *pad, float(fo.GAIN), 0.2, clamp, flip, nv.ptr(ps), nv.stream_of(src))
        torch.cuda.synchronize()
        y = out.float().cpu()
        assert torch.isfinite(y).all()
        return y

    # VALU: bf16 in / out with a bias
    x = (torch.randn(n, h, w, c_p, generator=g) * 3).bfloat16()
    b = torch.randn(c_p, generator=g)
    y = call("ic2_flrelu_nhwc", x.to(cuda), BF16, b.to(cuda), None, 5.0)
    r = _fwd_ref(x.permute(0, 3, 1, 2), fu, fd, b, up, pad, 5.0, flip)
    d = (y.permute(0, 3, 1, 2).double() - r).abs().max().item()
    assert d < 3e-2 * (1 + r.abs().max().item())
    # MFMA: f16 in, bf16 out, post_scale, clamp 256 reached
    x = (torch.randn(n, h, w, c_p, generator=g) * 2).half()
    x[:, :3, :5, :] = 300.0
    ps = torch.rand(n, c_p, generator=g) + 0.5
    y = call("ic2_flrelu_nhwc", x.to(cuda), F16, None, ps.to(cuda), 256.0)
    r = _fwd_ref(x.permute(0, 3, 1, 2), fu, fd, None, up, pad, 256.0, flip) * ps.double()[:, :, None, None]
    err = (y.permute(0, 3, 1, 2).double() - r).abs()
    assert err.max().item() < 2e-2 * (1 + r.abs().max().item())
    assert err.mean().item() < 2e-3 * (1 + r.abs().mean().item())
    xb = x.reshape(n, h, w, c_p // 16, 16).permute(0, 3, 1, 2, 4).contiguous()
    yb = call("ic2_flrelu_nhwc16", xb.to(cuda), F16, None, ps.to(cuda), 256.0)
    assert torch.equal(yb, y)
    del fua, fda


def test_zz_report_measured_ratios():
    """Prints the largest |got - ref| / (eps B) each path and tier reached over the cases above (the `measured` of the
    module docstring); the bars must not exceed the derived counts."""
    for (key, tier), v in sorted(RATIOS.items()):
        print(f"[flrelu-bwd-edges measured] {key} {tier}: max err/(eps B) {v:.3f}, bar {K_BAR[key]}, derived {K_DERIVED[key]}")
    assert all(K_BAR[k] <= K_DERIVED[k] for k in K_BAR)
