"""CPU: what training through a StyleGAN3-R generator adds, as far as it is checkable without a GPU: the cases of
tests/sg3r_bwd_cases.py (the mask tier's 20 % cap on the very inputs the GPU tests run, and the oracle's convention
for a 2-D down filter against loops), the C ABI's argument checks of ic2_flrelu_bwd_nhwc_2d, and the opt-in switch
Generator.set_radial_training.  The kernel is checked in tests/test_gpu_sg3r_train.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import flrelu_bwd_oracle as fo
import sg3r_bwd_cases as sc
from image_compression_2_amd import _native as nv
from image_compression_2_amd.networks_stylegan3 import Generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(z_dim=32, w_dim=32, img_resolution=32, num_layers=6, channel_base=256, channel_max=24)
GEOS = sc.geometries()
GEOS_R = sc.geometries(("r",))


# ------------------------------------------------------------------ the cases
def test_geometries_cover_the_tiles_and_both_phases():
    assert len(GEOS) == 2 * (len(sc.SIZES[2]) + len(sc.SIZES[4]))
    for gid, up, pad, h, w in GEOS:
        oh, ow = sc.out_size(h, w, up, pad)
        assert oh > 0 and ow > 0 and pad[0] == pad[2], gid
    for up in (2, 4):
        # the two paddings take the two gout phases: ph = (-(px0 - tu + 1 - td + 1)) mod 2
        assert {(-(p[0] - 6 * up + 1 - 12 + 1)) % 2 for p in sc.PADS[up].values()} == {0, 1}
        ty, tx = sc.TILE[up]
        hs, ws = {h for h, _ in sc.SIZES[up]}, {w for _, w in sc.SIZES[up]}
        assert any(h % ty == ty - 1 for h in hs) and any(h % ty == 0 for h in hs) and any(h % ty == 1 for h in hs)
        assert any(w % tx == tx - 1 for w in ws) and any(w % tx == 0 for w in ws) and any(w % tx == 1 for w in ws)


def _share(gid, up, pad, h, w, xdt, gdt, which, flip=1):
    fu, fd = sc.filters(up, which)
    x, gout, os_, b = sc.case_inputs(gid, up, pad, h, w, "mask", xdt, gdt)
    r = sc.reference(None, x, gout, fu, fd, up, pad, "mask", flip, os_, b, eps_x=sc.EPS_X_HOST)
    assert (r["B"] > 0).any() and torch.isfinite(r["ref"]).all()
    return (r["A"] > 0).double().mean().item()


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("geo", GEOS, ids=[g[0] for g in GEOS])
def test_mask_tier_allowance_on_at_most_a_fifth_f32(geo, flip):
    """The mask tier's condition on the reference alone, for the seeds the GPU sweep uses (f32 operands, the
    non-symmetric filters), at eps_x = 2^-11: the GPU test's eps_x = 2^-24 marks a subset of these elements.  Both
    flips: the GPU sweep runs flip 1 on the R paddings and both on the other gout phase, the fused-vs-composed and NULL
    cases flip 0, and the flip reverses the up filter, so U and the fragile set differ."""
    share = _share(*geo, sc.F32, sc.F32, "nonsym", flip)
    print(f"[sg3r-bwd-host] {geo[0]} f32 nonsym flip {flip}: A > 0 on {100 * share:.1f} %")
    assert share <= 0.20


@pytest.mark.parametrize("xdt,gdt", [t[:2] for t in sc.TRIPLES[1:]], ids=["f16_bf16", "f16_f16", "f16_f32"])
@pytest.mark.parametrize("geo", GEOS_R, ids=[g[0] for g in GEOS_R])
def test_mask_tier_allowance_on_at_most_a_fifth_16bit(geo, xdt, gdt):
    """The same for the 16-bit instances' stored operands on the R paddings (non-symmetric filters)."""
    share = _share(*geo, xdt, gdt, "nonsym")
    print(f"[sg3r-bwd-host] {geo[0]} {xdt}/{gdt} nonsym: A > 0 on {100 * share:.1f} %")
    assert share <= 0.20


@pytest.mark.parametrize("up", [2, 4])
def test_mask_tier_allowance_real_filters(up):
    """The real R-256 designs (L0_36_1024, L3_52_1024) on the case the GPU test runs them on."""
    gid, _, pad, h, w = REAL_GEO[up]
    for xdt, gdt, _ in sc.TRIPLES:
        assert _share(gid, up, pad, h, w, xdt, gdt, "r256", 0) <= 0.20   # the GPU test runs them with flip 0


REAL_GEO = {2: [g for g in GEOS_R if g[0] == "u2-r-17x33"][0], 4: [g for g in GEOS_R if g[0] == "u4-r-16x21"][0]}


def test_real_filters_are_the_r256_designs():
    for up in (2, 4):
        fu, fd = sc.r256_filters(up)
        assert fu.shape == (6 * up,) and fd.shape == (12, 12) and fd.dtype == torch.float32
        assert torch.allclose(fd, fd.t()) and abs(fd.double().sum().item() - 1) < 1e-6


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("up,h,w", [(2, 5, 7), (4, 13, 12)])
def test_oracle_2d_adjoint_matches_loops(up, h, w, flip):
    """fo.reference with a 2-D fd against the loop definition of the 2-D polyphase adjoint and the separable adjoint
    up FIR on one plane (slope 1, no clamp, non-symmetric filters): pins the oracle's convention for 2-D filters --
    flipped in both axes unless flip, row = y."""
    pad = sc.PADS[up]["r"]
    fu, fd = sc.nonsym_filters(up)
    oh, ow = sc.out_size(h, w, up, pad)
    g = torch.Generator().manual_seed(11 + up)
    x = torch.randn(1, h, w, 1, generator=g)
    gout = torch.randn(1, oh, ow, 1, generator=g)
    r = fo.reference(x, gout, fu, fd, up, pad, slope=1.0, clamp=-1.0, flip=flip, eps_x=sc.EPS_X, c=1)
    ref = r["ref"][0, :, :, 0]
    bf = sc.linear_backward_bruteforce(gout[0, :, :, 0].double(), fu.double(), fd.double(), up, pad, fo.GAIN, flip, h, w)
    assert ref.abs().max() > 0
    assert (bf - ref).abs().max().item() < 1e-12 * (1 + ref.abs().max().item())
    # the other flip is a different function of this filter
    other = sc.linear_backward_bruteforce(gout[0, :, :, 0].double(), fu.double(), fd.double(), up, pad, fo.GAIN,
                                          not flip, h, w)
    assert (other - ref).abs().max().item() > 1e-3 * ref.abs().max().item()
    # and so is the transposed table
    tr = sc.linear_backward_bruteforce(gout[0, :, :, 0].double(), fu.double(), fd.double().t().contiguous(), up, pad,
                                       fo.GAIN, flip, h, w)
    assert (tr - ref).abs().max().item() > 1e-3 * ref.abs().max().item()


# ------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_and_indexed():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(os.path.join(ROOT, "include", "ic2ops.h")).read()
    for name in ("ic2_flrelu_bwd_nhwc_2d", "ic2_flrelu_bwd_2d_ydot_floats"):
        assert f"`{name}`" in text and name in nv.exported_symbols() and re.search(r"\b%s\(" % name, hdr)
    assert nv.load().ic2_abi_version() == 1


def test_ydot_query_counts_the_kernels_tiles():
    for up in (2, 4):
        ty, tx = sc.TILE[up]
        for h, w in sc.SIZES[up]:
            want = 2 * -(-h // ty) * -(-w // tx) * 32
            assert int(nv.query("ic2_flrelu_bwd_2d_ydot_floats", 2, 32, h, w, up)) == want


def _call(**over):
    """One call of ic2_flrelu_bwd_nhwc_2d on a valid 16 x 16 x 16 problem (up 2, the R padding) with `over` applied
    -> (code, message).  Real device buffers where a GPU exists, dummy non-null addresses elsewhere."""
    fu = np.full(12, 1 / 12, np.float32)
    fd = np.full((12, 12), 1 / 144, np.float32)
    nyd = int(nv.query("ic2_flrelu_bwd_2d_ydot_floats", 1, 16, 16, 16, 2))
    if torch.cuda.is_available():
        bufs = [torch.zeros(1, 16, 16, 16, device="cuda") for _ in range(3)] + [torch.zeros(nyd, device="cuda")]
        x, g, gx, yd = (ctypes.c_void_p(t.data_ptr()) for t in bufs)
    else:
        x = g = gx = yd = ctypes.c_void_p(16)
    a = dict(x=x, xdt=nv.F32, g=g, gdt=nv.F32, gx=gx, odt=nv.F32, n=1, c_p=16, in_h=16, in_w=16, out_h=16, out_w=16, fu=fu,
             fu_taps=12, fd=fd, fd_taps=12, up=2, down=2, pad=(11, 10, 11, 10), ydot=yd, ydot_floats=nyd)
    a.update(over)
    fp = lambda v: None if v is None else v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib = nv.load()
    rc = lib.ic2_flrelu_bwd_nhwc_2d(a["x"], a["xdt"], a["g"], a["gdt"], a["gx"], a["odt"], a["n"], a["c_p"], a["in_h"],
                                    a["in_w"], a["out_h"], a["out_w"], fp(a["fu"]), a["fu_taps"], fp(a["fd"]),
                                    a["fd_taps"], a["up"], a["down"], *a["pad"], float(fo.GAIN), 0.2, 256.0, 0, None, None,
                                    a["ydot"], a["ydot_floats"], None)
    return rc, lib.ic2_last_error().decode()


INVALID, UNSUPPORTED = 1, 2


def test_bwd_2d_entry_point_refuses_before_any_launch():
    """Every refusal returns its code and a message before a kernel could be launched."""
    for null in ("x", "g", "gx", "fu", "fd"):
        rc, msg = _call(**{null: None})
        assert rc == INVALID and "null" in msg, null
    rc, msg = _call(out_h=17)
    assert rc == INVALID and "expected 16x16" in msg
    rc, msg = _call(out_w=15)
    assert rc == INVALID and "expected 16x16" in msg
    rc, msg = _call(pad=(11, 10, 10, 11))
    assert rc == UNSUPPORTED and "px0 == py0" in msg
    rc, msg = _call(fd_taps=11)
    assert rc == UNSUPPORTED and "no instance" in msg
    rc, msg = _call(fd_taps=13)
    assert rc == UNSUPPORTED and "no instance" in msg
    rc, msg = _call(up=3, fu_taps=18, fu=np.full(18, 1 / 18, np.float32))
    assert rc == UNSUPPORTED and "no instance" in msg
    rc, msg = _call(c_p=24)
    assert rc == UNSUPPORTED and "16" in msg
    # f16 gradients need f16 x, f16 gout and f16 gx; bf16 gradients need f16 x and a bf16 gx
    for xdt, gdt, odt in ((nv.F16, nv.F16, nv.BF16), (nv.F32, nv.F16, nv.F16), (nv.F16, nv.F32, nv.F16),
                          (nv.F16, nv.BF16, nv.F32), (nv.F32, nv.BF16, nv.BF16), (nv.BF16, nv.BF16, nv.BF16)):
        rc, msg = _call(xdt=xdt, gdt=gdt, odt=odt)
        assert rc == UNSUPPORTED and "dtypes" in msg, (xdt, gdt, odt)
    rc, msg = _call(ydot_floats=int(nv.query("ic2_flrelu_bwd_2d_ydot_floats", 1, 16, 16, 16, 2)) - 1)
    assert rc == INVALID and "ydot needs" in msg


def test_1x1_dgrad_runs_the_implicit_gemm():
    """The dgrad of a 1x1 layer is conv_nhwc(dc, packed_adjoint, k = 1, pad = 0): the launch plan never picks the
    Winograd kernel for k = 1, and has a plan for R's widest layers (1024 -> 1024 channels)."""
    for dt in (nv.F16, nv.BF16, nv.F32):
        for n, s, cin, cout in ((8, 36, 1024, 1024), (2, 36, 640, 384), (8, 276, 512, 384)):
            assert not nv.wino_preferred(dt, n, s, s, cin, cout, 1, 1, 0)
            odt = nv.F16_IEEE if dt == nv.F16 else dt
            assert nv.conv_plan(dt, odt, nv.NHWC, n, s, s, cin, cout, cout, 1, 1, 0)


# ------------------------------------------------------------------ the switch
def test_set_radial_training_sets_and_clears_every_flag():
    torch.manual_seed(0)
    G = Generator(**SMALL, conv_kernel=1, use_radial_filters=True).eval().requires_grad_(False)
    layers = G.synthesis.layers()
    assert G.synthesis.train_radial is False and all(L.train_radial is False for L in layers)
    assert G.set_radial_training() is G
    assert G.synthesis.train_radial is True and all(L.train_radial is True for L in layers)
    assert G.set_radial_training(False) is G
    assert G.synthesis.train_radial is False and all(L.train_radial is False for L in layers)


def test_switch_moves_the_cpu_call_from_the_refusal_to_the_device_check():
    """Unset: AutogradUnsupported before any launch, as before.  Set: the same call gets as far as the native path's
    device check, the way a T generator does."""
    torch.manual_seed(0)
    G = Generator(**SMALL, conv_kernel=1, use_radial_filters=True).eval().requires_grad_(False)
    T = Generator(**SMALL).eval().requires_grad_(False)
    ws = torch.randn(2, G.num_ws, G.w_dim, requires_grad=True)
    L = G.synthesis.layers()[0]
    x = torch.randn(2, L.in_channels, 36, 36, requires_grad=True)
    w = torch.randn(2, G.w_dim)
    with pytest.raises(nv.AutogradUnsupported, match="StyleGAN3-R"):
        G.synthesis(ws)
    with pytest.raises(nv.AutogradUnsupported, match="set_radial_training"):
        L(x, w)
    with pytest.raises(RuntimeError, match="ROCm devices only") as t_err:
        T.synthesis(ws)
    G.set_radial_training()
    try:
        with pytest.raises(RuntimeError, match="ROCm devices only") as r_err:
            G.synthesis(ws)
        assert type(r_err.value) is type(t_err.value) is RuntimeError
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            L(x, w)
    finally:
        G.set_radial_training(False)
    with pytest.raises(nv.AutogradUnsupported, match="StyleGAN3-R"):
        G.synthesis(ws)
