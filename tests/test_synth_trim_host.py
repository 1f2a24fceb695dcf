"""The read window of the filtered lrelu (ic2_flrelu_read_window), the trims the synthesis derives from it, and the
launch plans of the trimmed convs: host only.

* the native query against a brute-force 1-D reachability (one-hot inputs through zero-insert, pad / crop, all-ones
  FIRs of the given lengths, stride), for every layer of SG3-T-256 / -1024 and a sweep of small geometries;
* the identity the trims rest on, in fp64 on the oracle's functions: full conv + filtered lrelu against trimmed conv +
  shifted filtered lrelu per trimmed layer, and the chained L12 -> L13 case (bound 1e-12 max|ref|; measured: 0);
* the trimmed launch never plans more workgroups than the untrimmed one (C2 and C4 layers).
"""
import re

import pytest
import torch
import torch.nn.functional as F

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from oracle import sg3


def _reach(in_size, up, down, up_taps, down_taps, pad_lo, pad_hi):
    """R[i, o] > 0 iff input i reaches output o (fp64, one-hot inputs); None when the axis has no output."""
    x = torch.zeros(in_size, 1, in_size * up, dtype=torch.float64)
    x[torch.arange(in_size), 0, torch.arange(in_size) * up] = 1.0
    x = F.pad(x, (max(pad_lo, 0), max(pad_hi, 0)))
    x = x[..., max(-pad_lo, 0): x.shape[-1] - max(-pad_hi, 0)]
    if x.shape[-1] < up_taps + down_taps - 1:
        return None
    x = F.conv1d(x, torch.ones(1, 1, up_taps, dtype=torch.float64))
    x = F.conv1d(x, torch.ones(1, 1, down_taps, dtype=torch.float64))
    return x[:, 0, ::down]


def _span(mask):
    idx = torch.nonzero(mask).flatten()
    assert idx.numel() > 0 and idx.numel() == int(idx[-1] - idx[0]) + 1, "the reached inputs are one run"
    return int(idx[0]), int(idx[-1])


def _check_axis(in_size, up, down, up_taps, down_taps, pad_lo, pad_hi, ranges=None):
    R = _reach(in_size, up, down, up_taps, down_taps, pad_lo, pad_hi)
    if R is None:
        with pytest.raises(RuntimeError):
            nv.read_window(in_size, 1, up, down, up_taps, down_taps, pad_lo, pad_hi)
        return None
    out = R.shape[1]
    whole, _ = nv.read_window(in_size, out, up, down, up_taps, down_taps, pad_lo, pad_hi)
    assert whole == _span(R.sum(1) > 0), (in_size, up, pad_lo, pad_hi)
    for o0, o1 in ranges or [(0, out - 1), (out // 3, out - 1 - out // 4), (out - 1, out - 1), (0, 0)]:
        got = nv.read_window(in_size, out, up, down, up_taps, down_taps, pad_lo, pad_hi, o0, o1)
        assert got == (whole, _span(R[:, o0:o1 + 1].sum(1) > 0)), (in_size, up, pad_lo, pad_hi, o0, o1)
    return whole


@pytest.fixture(scope="module")
def gens():
    return {res: ic2.Generator(img_resolution=res, precision="f16") for res in (256, 1024)}


@pytest.mark.parametrize("res", [256, 1024])
def test_read_window_of_every_layer(gens, res):
    layers = gens[res].synthesis.layers()
    for L in layers:
        s_in, s_out, k = int(L.in_size[0]), int(L.out_size[0]), L.conv_kernel
        # the conv axis, and the filtered lrelu on the conv output
        assert _check_axis(s_in, 1, 1, k, 1, k - 1, k - 1) == (0, s_in - 1)
        whole = _check_axis(s_in + k - 1, L.up_factor, L.down_factor, L.up_taps, L.down_taps, *L.padding[:2])
        if L.up_factor == 4:
            assert whole == (2, s_in - 1), L.extra_repr()
        assert L.padding[:2] == L.padding[2:]
        assert L.unread_border() == (0 if L.is_torgb else min(whole[0], s_in + k - 2 - whole[1], k - 1))
    if res == 256:
        L12, L13 = layers[12], layers[13]
        assert nv.read_window(278, 256, 2, 2, 12, 12, *L13.padding[:2])[0] == (6, 271)
        # conv rows 6 .. 271 read L12's output rows 4 .. 271
        assert int(L12.out_size[0]) == 276 and nv.read_window(276, 278, 1, 1, 3, 1, 2, 2, 6, 271)[1] == (4, 271)
        assert [L.unread_border() for L in layers] == [0, 0, 0, 2, 0, 2, 0, 2, 0, 0, 2, 0, 0, 2, 0]


@pytest.mark.parametrize("up", [2, 4])
def test_read_window_sweep(up):
    """in 6 .. 40, taps 6 up / 12, down 2, paddings -12 .. 12 on both sides: equality is exact."""
    checked = 0
    for in_size in range(6, 41):
        for pad_lo in range(-12, 13):
            for pad_hi in range(-12, 13):
                checked += _check_axis(in_size, up, 2, 6 * up, 12, pad_lo, pad_hi) is not None
    assert checked > 0.8 * 35 * 25 * 25   # the rest are too short for one output, which the query reports


def test_read_window_rejects_bad_arguments():
    with pytest.raises(RuntimeError, match="does not match"):
        nv.read_window(38, 53, 4, 2, 24, 12, -6, -9)
    with pytest.raises(RuntimeError, match="outputs"):
        nv.read_window(38, 52, 4, 2, 24, 12, -6, -9, 3, 52)


# ------------------------------------------------------------------ the identity, fp64
def _layer_ref(L, x, w, conv_pad, padding):
    """conv (2 channels) + the layer's filtered lrelu in fp64."""
    y = F.conv2d(x, w, padding=conv_pad)
    return sg3.filtered_lrelu(y, L.up_filter.double(), L.down_filter.double(), None, up=L.up_factor,
                              down=L.down_factor, padding=padding, gain=2 ** 0.5, slope=0.2, clamp=256.0)


def _bound(got, want, what):
    assert got.shape == want.shape
    diff = (got - want).abs().max().item()
    print(f"{what}: max|diff| {diff:.3e} max|ref| {want.abs().max().item():.3e}")
    assert diff <= 1e-12 * want.abs().max().item()


@pytest.mark.parametrize("idx", [3, 5, 7, 10, 13])
def test_trim_identity_fp64(gens, idx):
    """Full conv + filtered lrelu against the conv without the unread border + the shifted filtered lrelu."""
    L = gens[256].synthesis.layers()[idx]
    T = L.trimmed(L.unread_border())
    assert T.border == 2 and T.conv_pad == 0
    g = torch.Generator().manual_seed(7 + idx)
    s_in = int(L.in_size[0])
    x = torch.randn(1, 2, s_in, s_in, generator=g, dtype=torch.float64)
    w = torch.randn(2, 2, 3, 3, generator=g, dtype=torch.float64)
    _bound(_layer_ref(L, x, w, T.conv_pad, T.flr_padding), _layer_ref(L, x, w, 2, L.padding), f"L{idx}")


def test_trim_identity_chained_fp64(gens):
    """L12 -> L13 with both trims (consumer: drop unread inputs, the padding grows by up each; producer: launch a
    range of outputs, the padding shrinks by down each): L12 writes only the 268^2 window L13's conv rows 6 .. 271
    read, L13's conv runs unpadded on it and its filtered lrelu gives the reference's 256^2.  Exact in fp64; the
    product does not launch L12 that way, because the strip kernel sums an output row's taps in an order that depends
    on the row's place in its 16-row tile, so a shifted output window changes the last bits."""
    L12, L13 = gens[256].synthesis.layers()[12:14]
    (c0, c1), _ = nv.read_window(278, 256, 2, 2, 12, 12, *L13.padding[:2])
    _, (i0, i1) = nv.read_window(276, 278, 1, 1, 3, 1, 2, 2, c0, c1)
    a, b = i0, 275 - i1
    assert (c0, c1, a, b) == (6, 271, 4, 4)
    pad12 = [L12.padding[0] - a * 2, L12.padding[1] - b * 2] * 2            # producer trim, down 2
    conv_pad = 2 + a - c0                                                    # both formulas on the conv axis
    pad13 = [L13.padding[0] + c0 * 2, L13.padding[1] + (277 - c1) * 2] * 2  # consumer trim, up 2
    assert pad12 == [1, 0, 1, 0] and conv_pad == 0 and pad13 == [1, 0, 1, 0]
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 2, 276, 276, generator=g, dtype=torch.float64)
    w12 = torch.randn(2, 2, 3, 3, generator=g, dtype=torch.float64)
    w13 = torch.randn(2, 2, 3, 3, generator=g, dtype=torch.float64)
    ref = _layer_ref(L13, _layer_ref(L12, x, w12, 2, L12.padding), w13, 2, L13.padding)
    mid = _layer_ref(L12, x, w12, 2, pad12)
    assert mid.shape[-1] == 268
    _bound(_layer_ref(L13, mid, w13, conv_pad, pad13), ref, "L12 -> L13")


# ------------------------------------------------------------------ launch plans
def _workgroups(L, n, s_in, pad):
    """Workgroups of the conv launch of layer L on an s_in^2 input with this padding, from the host planner's names
    (Winograd: tile pairs x rows; hg4: tile rows are not in the name -> the output pixels stand in, same instance or
    not); None where the name carries no tile."""
    out = s_in + 2 * pad - 2
    if nv.wino_preferred(nv.F16, n, s_in, s_in, L.cin_p, L.cout_p, 3, 3, pad):
        m = re.fullmatch(r"wino_fx_o128_p(\d+)x(\d+)(w?)_f16", nv.wino_plan(n, s_in, s_in, L.cin_p, L.cout_p, pad))
        twp, th = int(m.group(1)), int(m.group(2))   # tiles of twp pairs x th rows (tests/test_wino_plan.py, _cost)
        return "wino", n * -(-((out + 1) // 2) // twp) * -(-out // th) * -(-L.cout_p // 128)
    name = nv.conv_plan(nv.F16, nv.F16, nv.NHWC16, n, s_in, s_in, L.cin_p, L.cout_p, L.out_channels, 3, 3, pad)
    return name, n * out * out


@pytest.mark.parametrize("res,n,planned", [(256, 32, [5, 7]), (1024, 8, [])])
def test_trimmed_launch_plans_no_more_workgroups(gens, res, n, planned):
    """Every conv that could drop a border plans no more workgroups without it (C2 and C4 layers); the plan takes the
    Winograd layers whose rounds go down."""
    S = gens[res].synthesis
    for i, L in enumerate(S.layers()):
        T = L.trimmed(L.unread_border())
        if T is None:
            continue
        s_in = int(L.in_size[0])
        kind0, wg0 = _workgroups(L, n, s_in, 2)
        kind1, wg1 = _workgroups(L, n, s_in, T.conv_pad)
        rounds = [nv.wino_rounds(n, s_in, s_in, L.cin_p, L.cout_p, pad) for pad in (2, T.conv_pad)]
        print(res, i, kind0, wg0, "->", kind1, wg1, "wino rounds", rounds)
        assert wg1 <= wg0
        if kind0 == kind1 == "wino":
            assert rounds == [-(-wg // 256) for wg in (wg0, wg1)]
            assert (i in planned) == (rounds[1] < rounds[0])
        else:
            assert i not in planned
    assert [i for i, T in enumerate(S.trim_plan(n, torch.float16)) if T is not None] == planned
