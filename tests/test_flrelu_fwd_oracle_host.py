"""Pins tests/flrelu_fwd_oracle.py (reference, bound and case table of the filtered-lrelu forward edge tests) on the
CPU: the reference against the definition written as loops, the properties of B, an emulation of the kernels' f16
chain against the bound at the derived K on every MFMA case of the GPU table (so the reference alone never fails
it), and the coverage conditions on the very inputs the GPU cases run."""
import numpy as np
import pytest
import torch

import flrelu_bwd_oracle as fo
import flrelu_fwd_oracle as fw

BRUTE = {2: [9, 8, 11, 8], 4: [15, 14, 19, 14]}   # px0 != py0, same phase


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("up", [2, 4])
def test_forward_reference_matches_bruteforce(up, flip):
    """One 6 x 5 plane per up factor with a bias and a post_scale, a finite clamp that is reached, to 1e-12."""
    pad = BRUTE[up]
    fu, fd = fo.taps(up)
    g = torch.Generator().manual_seed(11 * up + flip)
    x = torch.randn(1, 6, 5, 1, generator=g, dtype=torch.float64) * 3
    x[0, 2, 1, 0] = 150.0
    b, ps = torch.tensor([0.75]), torch.tensor([[-1.25]])
    r = fw.forward_reference(x, fu, fd, up, pad, slope=0.2, clamp=50.0, flip=flip, bias=b, post_scale=ps)
    ref = fo.flrelu_bruteforce(x[0, :, :, 0] + 0.75, fu.double(), fd.double(), up, pad, fo.GAIN, 0.2, 50.0, bool(flip)) * -1.25
    assert r["ref"].shape[1:3] == ref.shape == fo.out_size(6, 5, up, pad)
    assert (r["ref"][0, :, :, 0] - ref).abs().max().item() < 1e-12 * (1 + ref.abs().max().item())
    assert r["ref"].abs().max().item() >= 50.0   # the clamp acted somewhere (|post_scale| > 1)
    other = fo.flrelu_bruteforce(x[0, :, :, 0] + 0.75, fu.double(), fd.double(), up, pad, fo.GAIN, 0.2, 50.0, not flip) * -1.25
    assert (other - ref).abs().max().item() > 1e-2 * ref.abs().max().item()


@pytest.mark.parametrize("up", [2, 4])
def test_B_dominates_and_ignores_signs(up):
    """|ref| <= B everywhere, for both tiers and flips; B is unchanged by sign changes of x, of the bias and of
    post_scale (the same under either flip), which do change ref."""
    name, h, w = fw.MATRIX[up]
    pad = fw.PADS[name][1]
    fu, fd = fo.taps(up)
    x = fw.mask_input(2, h, w, 5, 8, 3, torch.float64)
    ps, b = fo.scale_bias(2, 5, 8, 4)
    g = torch.Generator().manual_seed(5)
    sign = (torch.randint(0, 2, x.shape, generator=g) * 2 - 1).double()
    for tier, kw in fw.TIERS.items():
        for flip in (0, 1):
            r = fw.forward_reference(x, fu, fd, up, pad, flip=flip, bias=b, post_scale=ps, c=5, **kw)
            assert (r["ref"].abs() <= r["B"] * (1 + 1e-12)).all() and (r["B"] > 0).any()
            r2 = fw.forward_reference(x * sign, fu, fd, up, pad, flip=flip, bias=-b, post_scale=-ps, c=5, **kw)
            assert torch.equal(r2["B"], r["B"])
            assert not torch.equal(r2["ref"].abs(), r["ref"].abs())


def test_f16_round_taps_restatement():
    """Every rounded tap is one of the exact tap's two f16 neighbours, each group's sum error is no larger than with
    nearest rounding, and no scaled tap of the suite lies below 2^-15 (the count of the clamp-split K assumes it)."""
    for up in (2, 4):
        fu, fd = fo.taps(up)
        for flip in (0, 1):
            for clamp in (256.0, 1e4):
                for name, (ex, rd) in fw.kernel_taps(fu, fd, up, fo.GAIN, clamp, flip).items():
                    if name in ("guh", "gdgl") and not fw.clamp_split("strip", clamp):
                        continue
                    h = ex.astype(np.float16).astype(np.float32)
                    lo = np.minimum(h, np.where(h > ex, np.nextafter(h.astype(np.float16), np.float16(-np.inf)).astype(np.float32), h))
                    hi = np.maximum(h, np.where(h < ex, np.nextafter(h.astype(np.float16), np.float16(np.inf)).astype(np.float32), h))
                    assert ((rd == lo) | (rd == hi)).all(), (up, name)
                    assert (rd.astype(np.float16).astype(np.float32) == rd).all()
                    groups = up if name in ("gu", "guh") else 1
                    for p in range(groups):
                        e_joint = abs(float((rd[p::groups].astype(np.float64) - ex[p::groups]).sum()))
                        e_near = abs(float((h[p::groups].astype(np.float64) - ex[p::groups]).sum()))
                        assert e_joint <= e_near + 1e-12
                    assert np.abs(ex).min() >= 2.0 ** -15, (up, name, np.abs(ex).min())
                    ulp = 4.0 if np.abs(ex).min() < 2.0 ** -14 else 2.0
                    assert (np.abs(rd.astype(np.float64) - ex) <= ulp * 2.0 ** -11 * np.abs(ex)).all(), (up, name)


RATIOS = {}


@pytest.mark.parametrize("path", fw.PATHS)
def test_sweep_cases_reference_coverage_and_emulation(path, capsys):
    """On the inputs of every case of the GPU sweep (same builders), both tiers:
    * the median of |ref| / B is at least 0.03, so the bound is a few percent of a typical value;
    * mask tier: between 3 % and 35 % of the grid positions of the clamp channels (the first third) sit at the clamp,
      and both lrelu sides hold at least 30 % of the positions.  The window holds per case wherever the input has at
      least 6 samples per axis (one full polyphase set of up taps), and for the path's mean over its cases.  The strip
      sweep's one-row and one-column outputs at up 2 come from inputs 2 or 3 samples high or wide, where no grid
      position sees six samples and the pre-activation stays smaller: 1.3 .. 2.6 % of their positions clamp (eight
      cases); at least 1 % is asserted for inputs under 6 samples on an axis;
    * MFMA paths: the torch emulation of the f16 chain meets the bound at the derived K."""
    lines, shares = [], []
    for case in fw.sweep_cases(path):
        up, pad = case["up"], case["pad"]
        fu, fd = fo.taps(up)
        for tier, kw in fw.TIERS.items():
            x, b, ps, c = fw.case_inputs(case, tier)
            r = fw.forward_reference(x, fu, fd, up, pad, flip=case["flip"], bias=b, post_scale=ps, c=c, **kw)
            live = r["B"] > 0
            med = (r["ref"].abs()[live] / r["B"][live]).median().item()
            msg = f"[flrelu-fwd host] {path} {case['id']} {tier}: median |ref|/B {med:.3f}"
            assert med >= 0.03, msg
            if tier == "mask":
                share = r["clamped"][: c // 3].mean().item()
                msg += f", clamped {100 * share:.1f} %, positive {100 * r['positive']:.1f} %"
                shares.append(share)
                if min(case["in_h"], case["in_w"]) >= 6:
                    assert 0.03 <= share <= 0.35, msg
                else:
                    assert 0.01 <= share <= 0.35, msg
                assert 0.30 <= r["positive"] <= 0.70, msg
                assert r["clamped"][c // 3:].max().item() == 0.0, msg
            if path in ("strip", "tile"):
                split = fw.clamp_split(path, kw["clamp"])
                got = fw.emulate_f16_chain(x, fu, fd, up, pad, fo.GAIN, kw["slope"], kw["clamp"], case["flip"], ps,
                                           fw.BF16, split, c)
                K = fw.K_DERIVED_CLAMP_SPLIT if split else fw.K_DERIVED[fw.KEY[path]]
                F = fw.floor_f16(path, fu, fd, up, fo.GAIN, kw["clamp"], ps, fw.BF16, case["xdt"], x.shape[0], c)
                err = (got - r["ref"]).abs()
                assert (err <= fw.bound(r, K, 2.0 ** -11, fw.BF16, F)).all(), msg
                ratio = ((err - F).clamp_min(0)[live] / (2.0 ** -11 * r["B"][live])).max().item()
                RATIOS[path, tier] = max(RATIOS.get((path, tier), 0.0), ratio)
                msg += f", emulation max err/(eps B) {ratio:.2f}"
            lines.append(msg)
    mean = sum(shares) / len(shares)
    assert 0.03 <= mean <= 0.35, mean
    with capsys.disabled():
        print("\n" + "\n".join(lines))
        print(f"[flrelu-fwd host] {path} mask: clamped {100 * min(shares):.1f} .. {100 * max(shares):.1f} %, mean {100 * mean:.1f} %")
        for (p, t), v in sorted(RATIOS.items()):
            if p == path:
                print(f"[flrelu-fwd host] {p} {t}: emulation (bf16 out) worst err/(eps B) {v:.2f}")


def test_every_instance_reached():
    """Every (kernel, up, delta) instance is reached by at least one (asymmetric-tap) sweep case: (2,0), (2,1) and
    (4,0) .. (4,3) for the strip, the tile and each VALU instance family; flips 0 and 1 and, on the strip, both input
    layouts too; no output is square and every padding has px0 = py0 (mod up)."""
    want = {(2, 0), (2, 1), (4, 0), (4, 1), (4, 2), (4, 3)}
    for path in fw.PATHS:
        cases = fw.sweep_cases(path)
        assert len({c["id"] for c in cases}) == len(cases)
        for flip in (0, 1):
            assert {(c["up"], c["pad"][0] % c["up"]) for c in cases if c["flip"] == flip} == want, path
        if path == "strip":
            for bl in (False, True):
                assert {(c["up"], c["pad"][0] % c["up"]) for c in cases if c["blocked_in"] == bl} == want
        if path == "nchw":
            for dt in (fw.F32, fw.BF16):
                assert {(c["up"], c["pad"][0] % c["up"]) for c in cases if c["xdt"] == dt} == want
        for c in cases:
            oh, ow = fo.out_size(c["in_h"], c["in_w"], c["up"], c["pad"])
            assert oh > 0 and ow > 0 and oh != ow and (c["pad"][0] - c["pad"][2]) % c["up"] == 0
    assert any(c["pad"][0] != c["pad"][2] for c in fw.sweep_cases("strip"))
    for up in (2, 4):
        fu, fd = fo.taps(up)
        assert (fu - fu.flip(0)).abs().max() > 0.01 and (fd - fd.flip(0)).abs().max() > 0.01 and fd.numel() == 12
    # the strip sweep's sizes: widths around the 32-column strip, last-tile live rows around tail_skip's 11
    for up, lives, widths in ((2, {1, 11, 12, 16}, {1, 31, 32, 33}), (4, {2, 10, 12, 16}, {2, 30, 32, 34})):
        got = [fo.out_size(c["in_h"], c["in_w"], up, c["pad"]) for c in fw.sweep_cases("strip")
               if c["up"] == up and c["pad"][0] > 0]
        assert {(oh - 1) % 16 + 1 for oh, _ in got} == lives and {ow for _, ow in got} == widths
        for live in lives:
            assert {-(-oh // 16) for oh, _ in got if (oh - 1) % 16 + 1 == live} == {1, 2}


@pytest.mark.parametrize("resident", [512, 1024])
@pytest.mark.parametrize("up", [2, 4])
def test_chained_cases_reach_the_chained_code(up, resident):
    """fm_strip_segments / fm_strip_grid restated, at 256 CUs x 2 and x 4 resident workgroups (the occupancy is not
    queryable from Python): every chained case keeps whole strips of at least 2 tiles, has more items than resident
    workgroups (has_next, the next item's prefetch) and its blocks reach k = 3 (the counted store waits, MODE 2);
    the last tile's live rows sit on both sides of tail_skip's threshold.  The small sweep cases do not get there:
    each of their tiles is its own item."""
    lives = set()
    for oh_t in fw.CHAIN_OUT_H:
        in_h, oh = fw.chain_in_h(up, oh_t)
        assert fo.out_size(in_h, fw.CHAIN_W, up, fw.CHAIN_PAD[up])[0] == oh
        ow = fo.out_size(in_h, fw.CHAIN_W, up, fw.CHAIN_PAD[up])[1]
        assert 0 < ow <= 32   # tiles_x = 1
        tiles_y = -(-oh // 16)
        assert 3 <= tiles_y <= 5
        nstrips = fw.CHAIN_N * 1 * (fw.CHAIN_CP // 16)
        assert nstrips == 2048
        sg = fw.strip_grid(nstrips, tiles_y, resident)
        assert sg["seg_len"] >= 2 and sg["nitems"] > resident, sg
        live = oh - 16 * (tiles_y - 1)
        lives.add(live)
        nt = min(sg["seg_len"], tiles_y - (sg["nseg"] - 1) * sg["seg_len"])   # the item that ends the strip
        kend = 2 * nt - (1 if live <= 11 else 0)
        assert sg["seg_len"] >= 2 and 2 * sg["seg_len"] - 1 >= 3 and (nt < 2 or kend >= 3), (sg, nt, kend)
    assert min(lives) <= 11 and 12 in lives and 16 in lives
    for case in fw.sweep_cases("strip"):
        oh, ow = fo.out_size(case["in_h"], case["in_w"], case["up"], case["pad"])
        sg = fw.strip_grid(fw.N * -(-ow // 32) * 2, -(-oh // 16), resident)
        assert sg["seg_len"] == 1 and sg["nitems"] <= resident


@pytest.mark.parametrize("up", [2, 4])
def test_replicated_cases_inputs(up):
    """The scale pattern separates neighbouring samples and channel blocks; in the mask tier the scale-1 copy of the
    chained input keeps the clamp share inside the sweep's window (the other scales are printed: their references are
    computed per scale by the GPU test, not by scaling); f16 never overflows at scale 4."""
    idx = fw.scale_index(fw.CHAIN_N, fw.CHAIN_CP // 16)
    assert (idx[1:] != idx[:-1]).all() and (idx[:, 1:] != idx[:, :-1]).all()
    assert {int(v) for v in idx.unique()} == {0, 1, 2, 3}
    fu, fd = fo.taps(up)
    in_h, _ = fw.chain_in_h(up, fw.CHAIN_OUT_H[0])
    x1, ps, _ = fw.replicated_inputs(up, "mask", in_h, fw.CHAIN_W, fw.CHAIN_N, fw.CHAIN_CP, fw.F16, 40)
    assert x1.abs().max().item() * 4 * 2 < 65504
    assert len({float(v) for v in ps.flatten()[:64]}) == 64
    for s in fw.SCALES:
        r = fw.forward_reference(x1 * s, fu, fd, up, fw.CHAIN_PAD[up], **fw.TIERS["mask"])
        share = r["clamped"][:5].mean().item()
        print(f"[flrelu-fwd host] chained u{up} scale {s}: clamped {100 * share:.1f} %")
        if s == 1.0:
            assert 0.03 <= share <= 0.35
