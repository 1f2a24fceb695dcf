"""Pins tests/flrelu_bwd_oracle.py (the fp64 reference of the filtered-lrelu backward edge tests) on the CPU:
sg3's tap-order conventions against a brute-force loop, the autograd reference against finite differences, the
bound / allowance properties, and the mask-tier condition (at most 20 % of the elements carry a mask allowance) on
the inputs of every GPU case."""
import pytest
import torch

import flrelu_bwd_oracle as fo
from oracle import sg3


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("up,padding,h,w", [(2, [9, 8, 9, 10], 4, 3), (4, [-6, -9, -6, -9], 13, 14)])
def test_sg3_tap_order_matches_bruteforce(up, padding, h, w, flip):
    """upfirdn2d and filtered_lrelu with asymmetric taps, flip_filter off and on, against the definition written as
    loops; the two tap orders must differ (the taps are asymmetric), so a reversed filter cannot pass."""
    fu, fd = fo.taps(up)
    g = torch.Generator().manual_seed(up + int(flip))
    x = torch.randn(h, w, generator=g, dtype=torch.float64) * 3
    got = sg3.upfirdn2d(x[None, None], fu.double(), up=up, padding=padding, gain=up ** 2, flip_filter=flip)[0, 0]
    ref = fo.upfirdn_bruteforce(x, fu.double(), up, 1, padding, flip, gain=up ** 2)
    other = fo.upfirdn_bruteforce(x, fu.double(), up, 1, padding, not flip, gain=up ** 2)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < 1e-12 * (1 + ref.abs().max().item())
    assert (other - ref).abs().max().item() > 1e-2 * ref.abs().max().item()
    v = torch.randn(13, 16, generator=g, dtype=torch.float64)
    got = sg3.upfirdn2d(v[None, None], fd.double(), down=2, flip_filter=flip)[0, 0]
    ref = fo.upfirdn_bruteforce(v, fd.double(), 1, 2, [0, 0, 0, 0], flip)
    assert got.shape == ref.shape and (got - ref).abs().max().item() < 1e-12
    x[0, 0] = 150.0   # reaches the clamp
    got = sg3.filtered_lrelu(x[None, None], fu.double(), fd.double(), None, up=up, down=2, padding=padding,
                             gain=fo.GAIN, slope=0.2, clamp=50.0, flip_filter=flip)[0, 0]
    ref = fo.flrelu_bruteforce(x, fu.double(), fd.double(), up, padding, fo.GAIN, 0.2, 50.0, flip)
    assert got.shape == ref.shape == fo.out_size(h, w, up, padding)
    assert (got - ref).abs().max().item() < 1e-11 * (1 + ref.abs().max().item())


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("up,padding,h,w", [(2, [10, 9, 10, 9], 5, 4), (4, [15, 14, 15, 14], 3, 4)])
def test_reference_matches_finite_differences(up, padding, h, w, flip):
    """ref, ydot, B and A of the helper on a tiny case: ref against central differences of the (piecewise linear)
    forward, B >= |ref| everywhere, A >= 0, and A = 0 exactly when no position is fragile (the linear tier)."""
    fu, fd = fo.taps(up)
    g = torch.Generator().manual_seed(7 * up + int(flip))
    n, c = 2, 3
    x = torch.randn(n, h, w, c, generator=g, dtype=torch.float64) * 4
    x[0, 1, 1, 0] = 300.0
    oh, ow = fo.out_size(h, w, up, padding)
    gout = torch.randn(n, oh, ow, c, generator=g, dtype=torch.float64)
    os_, b = fo.scale_bias(n, c, c, 5)
    for tier, kw in fo.TIERS.items():
        r = fo.reference(x, gout, fu, fd, up, padding, flip=flip, oscale=os_, bias=b, eps_x=2.0 ** -11, **kw)

        def loss(xx):
            o = sg3.filtered_lrelu(xx.permute(0, 3, 1, 2), fu.double(), fd.double(), None, up=up, down=2,
                                   padding=padding, gain=fo.GAIN, slope=kw["slope"],
                                   clamp=None if kw["clamp"] < 0 else kw["clamp"], flip_filter=flip)
            return (o * gout.permute(0, 3, 1, 2)).sum().item()

        fd_grad = torch.zeros_like(x)
        step = 1e-6
        for i in range(x.numel()):
            e = torch.zeros(x.numel(), dtype=torch.float64)
            e[i] = step
            e = e.view_as(x)
            fd_grad.view(-1)[i] = (loss(x + e) - loss(x - e)) / (2 * step)
        scale = fd_grad.abs().max().item()
        assert (r["ref0"] - fd_grad).abs().max().item() < 1e-6 * scale, tier
        assert torch.equal(r["ref"], r["ref0"] * os_.double()[:, None, None, :])
        yd = (fd_grad * (x - b.double())).sum(dim=(1, 2))
        assert (r["ydot"] - yd).abs().max().item() < 1e-6 * (1 + yd.abs().max().item())
        assert (r["B"] >= r["ref"].abs() * (1 - 1e-12)).all()
        assert (r["A"] >= 0).all()
        if tier == "linear":
            assert r["fragile"] == 0.0 and r["A"].abs().max().item() == 0.0
    # a pre-activation placed on the lrelu kink makes its neighbourhood fragile, and only then A > 0
    z = torch.zeros(1, h, w, 1, dtype=torch.float64)
    r = fo.reference(z + 1.0, gout[:1, :, :, :1].abs() + 1, fu, fd, up, padding, flip=flip)
    assert r["fragile"] > 0 or r["A"].abs().max().item() == 0.0
    r = fo.reference(z + 1.0, gout[:1, :, :, :1].abs() + 1, fu, fd, up, padding, flip=flip, kappa=0.0)
    assert r["fragile"] == 0.0 and r["A"].abs().max().item() == 0.0


def test_builders():
    """The taps are asymmetric and normalised; the block-sign input is what its docstring says; the geometry list
    has every listed side with every padding and no square input."""
    for up in (2, 4):
        fu, fd = fo.taps(up)
        assert fu.numel() == 6 * up and fd.numel() == 12
        assert abs(fu.double().sum().item() - 1) < 1e-6 and abs(fd.double().sum().item() - 1) < 1e-6
        assert (fu - fu.flip(0)).abs().max() > 0.01 and (fd - fd.flip(0)).abs().max() > 0.01
        fs, _ = fo.taps(up, asym=False)
        assert (fs - fs.flip(0)).abs().max() < 1e-7
    x = fo.block_sign_input(2, 17, 9, 22, 32, 3, torch.float16).double()
    assert (x[..., 22:] == 0).all() and (x[..., :22].abs() >= 4 - 1e-2).all()
    assert (x[..., :7].abs() >= 160 - 1).all() and x[..., 7:22].abs().max() < 40
    assert (x[0, :8, :8, 5].sign() == x[0, 0, 0, 5].sign()).all()
    assert not torch.equal(x[0], x[1])
    geo = fo.geometries()
    assert len({g[0] for g in geo}) == len(geo)
    for gid, up, pad, h, w in geo:
        oh, ow = fo.out_size(h, w, up, pad)
        assert h != w and oh > 0 and ow > 0 and pad[0] == pad[2], gid
    for pads, sizes, up in ((fo.UP2_PADS, fo.UP2_SIZES, 2), (fo.UP4_PADS, fo.UP4_SIZES, 4)):
        for pad in pads.values():
            hs = {h for _, u, p, h, w in geo if u == up and p == pad}
            ws = {w for _, u, p, h, w in geo if u == up and p == pad}
            if pad[0] > 0:
                assert hs == {h for h, _ in sizes} and ws == {w for _, w in sizes}
    assert {h for h, _ in fo.UP2_SIZES} == {5, 15, 16, 17, 31, 33} and {w for _, w in fo.UP2_SIZES} == {7, 15, 16, 17, 33}
    assert {h for h, _ in fo.UP4_SIZES} == {5, 15, 16, 17, 31, 33} and {w for _, w in fo.UP4_SIZES} == {3, 7, 8, 9, 17, 21}
    # out_h != out_w from the padding alone, and both R phases per up factor (R = 11 - (p0 mod 2) for these taps)
    assert {p[0] % 2 for p in fo.UP2_PADS.values()} == {0, 1} and {p[0] % 2 for p in fo.UP4_PADS.values()} == {0, 1}


@pytest.mark.parametrize("path", ["mfma", "valu"])
def test_mask_tier_allowance_share(path, capsys):
    """The mask-tier condition of tests/test_gpu_flrelu_bwd_edges.py: on the inputs of every GPU case (same builders),
    at most 20 % of the valid-channel elements carry a mask allowance A > 0 -- from the reference alone."""
    lines, worst = [], 0.0
    cases = [(gid, up, pad, fo.case_inputs(gid, up, pad, h, w, path, "mask"), fo.C, (0, 1))
             for gid, up, pad, h, w in fo.geometries()]
    if path == "mfma":   # the chained-strip cases (MFMA only, flip 0)
        cases += [(f"chained-u{up}", up, fo.CHAINED[up][0], fo.chained_inputs(up, "mask"), fo.CHAINED_C, (0,))
                  for up in (2, 4)]
    for gid, up, pad, (x, gout, os_, b), c, flips in cases:
        fu, fd = fo.taps(up)
        for flip in flips:
            r = fo.reference(x, gout, fu, fd, up, pad, flip=flip, oscale=os_, bias=b, eps_x=fo.EPS_X[path], c=c,
                             **fo.TIERS["mask"])
            share = (r["A"] > 0).double().mean().item()
            worst = max(worst, share)
            lines.append(f"[flrelu-bwd mask share] {path} {gid} flip {flip}: A > 0 on {100 * share:.1f} % "
                         f"(fragile grid positions {100 * r['fragile']:.2f} %)")
            assert share <= 0.20, lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines) + f"\n[flrelu-bwd mask share] {path}: worst {100 * worst:.1f} %")


@pytest.mark.parametrize("gid", ["u2-p9_8_9_10-17x33", "u4-p15_14-17x9", "u4-crop6_9-17x21"])
def test_mask_tier_bound_rejects_reference_side_mutants(gid):
    """The mask-tier bound of the bf16 MFMA path (the loosest of the GPU file: K 9, eps 2^-9, eps_out 2^-8, A at
    eps_x 2^-11) still rejects wrong results: references computed with the taps reversed, slope 0.25, the last gout
    row or column dropped and the last x row read as 0 each exceed it on at least 0.1 % of the elements (one is
    enough to fail a GPU case) -- except the
    last x row under a crop, which reaches no output and must change nothing."""
    _, up, pad, h, w = [g for g in fo.geometries() if g[0] == gid][0]
    fu, fd = fo.taps(up)
    x, gout, os_, b = fo.case_inputs(gid, up, pad, h, w, "mfma", "mask")
    kw = dict(oscale=os_, bias=b, eps_x=fo.EPS_X["mfma"], c=fo.C)
    r = fo.reference(x, gout, fu, fd, up, pad, flip=False, **kw)
    bound = 9 * 2.0 ** -9 * r["B"] + 2.0 ** -8 * r["ref"].abs() + r["A"]
    g_row, g_col, x_row = gout.clone(), gout.clone(), x.clone()
    g_row[:, -1] = 0
    g_col[:, :, -1] = 0
    x_row[:, -1] = 0
    mutants = {"taps reversed": fo.reference(x, gout, fu, fd, up, pad, flip=True, **kw),
               "slope 0.25": fo.reference(x, gout, fu, fd, up, pad, flip=False, slope=0.25, **kw),
               "last gout row": fo.reference(x, g_row, fu, fd, up, pad, flip=False, **kw),
               "last gout column": fo.reference(x, g_col, fu, fd, up, pad, flip=False, **kw),
               "last x row": fo.reference(x_row, gout, fu, fd, up, pad, flip=False, **kw)}
    for name, m in mutants.items():
        over = ((m["ref"] - r["ref"]).abs() > bound).double().mean().item()
        print(f"[flrelu-bwd bound] {gid} {name}: over the bound on {100 * over:.1f} % of the elements")
        if name == "last x row" and pad[0] < 0:
            assert torch.equal(m["ref"][:, :-1], r["ref"][:, :-1])
        else:
            assert over >= 0.001, (gid, name, over)
