"""Trimmed synthesis launches and the strip kernel's skipped tail block (GPU).

The strip filtered-lrelu kernel drops the last 16-row grid block of a strip whose last tile has at most 11 live rows:
checked against the fp64 composition (at test_gpu_kernels.py's bars for this kernel), bit for bit against a taller
launch of the same input in which the compared tiles are not last, and with guard bands around the output.  The
no-grad 16-bit synthesis runs convs without the border their filtered lrelu never reads: bit-equal to the reference
geometry, per layer and for the whole network.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from image_compression_2_amd import networks_stylegan3 as ns
from oracle import sg3

pytestmark = pytest.mark.gpu

GUARD = 8192
SENTINEL = 0x7E5A  # a NaN in f16 and in bf16: no output of the kernel has these bits


def _axis(out, up, p0):
    """(in, p1) of an axis with `out` outputs, leading padding p0, 6 * up / 12 taps, down 2: the shortest input whose
    trailing padding is <= 0 (up 4, SG3's cropping layers) or SG3's 8 (up 2)."""
    need = 2 * (out - 1) + 1 + 6 * up + 12 - 2
    if up == 2:
        size = (need - p0 - 8) // 2
    else:
        size = -(-(need - p0) // up)
    return size, need - size * up - p0


def _filters(up):
    fu = sg3.design_lowpass_filter(6 * up, 8.0, 4.0, 64)
    fd = sg3.design_lowpass_filter(12, 8.0, 4.0, 64)
    return fu, fd


def _launch(xb, n, c_p, in_h, in_w, out_h, out_w, up, pad, fu, fd, ps, blocked_out, dev):
    """ic2_flrelu_nhwc16, f16 -> f16, into a guarded buffer: -> (NHWC output, guards intact?, every element written?)."""
    numel = n * out_h * out_w * c_p
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=dev)
    out = buf[GUARD:GUARD + numel].view(torch.float16)
    fun, fdn = fu.float().contiguous().numpy(), fd.float().contiguous().numpy()
    nv.call("ic2_flrelu_nhwc16", nv.ptr(xb), ctypes.c_void_p(out.data_ptr()), nv.F16,
            nv.F16 | (nv.flr_out_layout(nv.NHWC16) if blocked_out else 0), n, c_p, in_h, in_w, out_h, out_w,
            fun.ctypes.data_as(ctypes.c_void_p), fun.shape[0], fdn.ctypes.data_as(ctypes.c_void_p), fdn.shape[0], None,
            up, 2, *pad, float(np.sqrt(2)), 0.2, 256.0, 0, nv.ptr(ps), nv.stream_of(xb))
    torch.cuda.synchronize()
    guards = bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + numel:] == SENTINEL).all())
    written = bool((buf[GUARD:GUARD + numel] != SENTINEL).all())
    if blocked_out:
        y = out.view(n, c_p // 16, out_h, out_w, 16).permute(0, 2, 3, 1, 4).reshape(n, out_h, out_w, c_p)
    else:
        y = out.view(n, out_h, out_w, c_p)
    return y.clone(), guards, written


def _check_strip(dev, n, c_p, out_h, out_w, up, blocked_out, ref_channels=None):
    p0 = 9 if up == 2 else 2
    in_h, py1 = _axis(out_h, up, p0)
    in_w, px1 = _axis(out_w, up, p0)
    g = torch.Generator().manual_seed(1000 * up + 10 * out_h + c_p % 7)
    x = (torch.randn(n, c_p, in_h, in_w, generator=g) * 2).half()
    x[:, :, :2, :3] = 300.0  # exercises the clamp
    ps = torch.rand(n, c_p, generator=g) + 0.5
    xb = x.view(n, c_p // 16, 16, in_h, in_w).permute(0, 1, 3, 4, 2).contiguous().to(dev)
    psd = ps.to(dev)
    fu, fd = _filters(up)
    y, guards, written = _launch(xb, n, c_p, in_h, in_w, out_h, out_w, up, [p0, px1, p0, py1], fu, fd, psd,
                                 blocked_out, dev)
    assert guards, "the kernel wrote outside its output"
    assert written, "an output element was not written"
    # taller launch: 16 more output rows from 32 more rows of trailing padding; the compared tiles are not its last
    tall, guards, written = _launch(xb, n, c_p, in_h, in_w, out_h + 16, out_w, up, [p0, px1, p0, py1 + 32], fu, fd, psd,
                                    blocked_out, dev)
    assert guards and written
    assert torch.equal(y, tall[:, :out_h]), "rows differ from the launch in which no block is skipped"
    # fp64 composition, test_gpu_kernels.py::test_flrelu_nhwc_bf16_matches_oracle's bars (f16 output)
    ch = slice(None) if ref_channels is None else ref_channels
    r = sg3.filtered_lrelu(x[:, ch].double(), fu.double(), fd.double(), None, up=up, down=2,
                           padding=[p0, px1, p0, py1], gain=np.sqrt(2), slope=0.2, clamp=256.0)
    r = r * ps[:, ch].double()[:, :, None, None]
    got = y.float().cpu().permute(0, 3, 1, 2)[:, ch]
    assert got.shape == r.shape
    err = (got.double() - r).abs()
    scale = r.abs().max().item()
    print(f"out_h {out_h} up {up} c_p {c_p} blocked {blocked_out}: max err {err.max().item():.3e} mean "
          f"{err.mean().item():.3e} scale {scale:.3e}")
    assert err.max().item() < 2e-2 * (1 + scale), (err.max().item(), scale)
    assert err.mean().item() < 2e-3 * (1 + r.abs().mean().item())
    assert err.max().item() < 4e-3 * (1 + scale), (err.max().item(), scale)


@pytest.mark.parametrize("blocked_out", [False, True])
@pytest.mark.parametrize("up", [2, 4])
@pytest.mark.parametrize("c_p", [16, 32])
@pytest.mark.parametrize("out_h", [4, 11, 12, 20, 27, 28])
def test_strip_tail_block(cuda, out_h, c_p, up, blocked_out):
    """One tile with (4, 11) and without (12) the skip, and 4 / 11 / 12 live rows behind a full tile (20, 27, 28); few
    strips, so the launch is segmented."""
    _check_strip(cuda, 1, c_p, out_h, 36, up, blocked_out)


@pytest.mark.parametrize("blocked_out", [False, True])
def test_strip_tail_block_unsegmented(cuda, blocked_out):
    """Enough strips (4 x 2 x 128) that every strip is one item.  The fp64 composition is evaluated on three
    16-channel blocks (first, middle, last); the other two checks cover every channel."""
    ch = torch.cat([torch.arange(0, 16), torch.arange(1024, 1040), torch.arange(2032, 2048)])
    _check_strip(cuda, 4, 2048, 20, 64, 2, blocked_out, ref_channels=ch)


# ------------------------------------------------------------------ layers and network
@pytest.fixture(scope="module")
def gens(cuda):
    torch.manual_seed(3)
    G = ic2.Generator(img_resolution=256, precision="f16").to(cuda).eval().requires_grad_(False)
    return G


def _synth(G, ws, on):
    old = ns._SYNTH_TRIM
    ns._SYNTH_TRIM = on
    try:
        with torch.no_grad():
            img = G.synthesis(ws)
        torch.cuda.synchronize()
        return img
    finally:
        ns._SYNTH_TRIM = old


@pytest.mark.parametrize("precision,n", [("f16", 2), ("bf16", 1), ("f16", 32)])
def test_synthesis_trimmed_equals_reference_geometry(cuda, gens, precision, n):
    """The image with the switch on and off.  The plan trims where a conv saves a round of workgroups: nowhere at the
    small batches, L5 and L7 at the benchmark's 32."""
    G = gens.set_precision(precision)
    try:
        ws = torch.randn(n, G.num_ws, G.w_dim, generator=torch.Generator().manual_seed(5)).to(cuda)
        on, off = _synth(G, ws, True), _synth(G, ws, False)
        plan = G.synthesis.trim_plan(n, nv.torch_dtype(precision))
        assert [i for i, t in enumerate(plan) if t is not None] == ([5, 7] if n == 32 else [])
        assert torch.isfinite(on).all() and on.shape == (n, 3, 256, 256)
        assert torch.equal(on, off)
    finally:
        gens.set_precision("f16")


@pytest.mark.parametrize("idx", [[3], [5], [13], [12, 13]])
def test_layers_trimmed_equal_reference_geometry(cuda, gens, idx):
    """run_nhwc of a layer with and without its conv's unread border, bit for bit, at n = 1: L3 (implicit GEMM, the
    same K split at this batch), L5 (Winograd), L13 (hg4), and L13 behind L12.  (L12 itself always writes its whole
    276^2: launched on the 268^2 window L13 reads, the strip kernel sums some taps in another order and the last bits
    change, so that trim is not in the product.)"""
    layers = gens.synthesis.layers()
    dt, n = torch.float16, 1
    g = torch.Generator().manual_seed(40 + idx[0])
    L0 = layers[idx[0]]
    s_in = int(L0.in_size[0])
    x = torch.zeros(n, s_in, s_in, L0.cin_p)
    x[..., :L0.in_channels] = torch.randn(n, s_in, s_in, L0.in_channels, generator=g)
    ref = got = x.to(cuda, dt)
    with torch.no_grad():
        for i in idx:
            L = layers[i]
            T = L.trimmed(L.unread_border())
            assert (T is None) == (i == 12)
            osc = (torch.rand(n, L.cout_p, generator=g) * 0.04 + 0.02).to(cuda)
            post = (torch.rand(n, L.cout_p, generator=g) + 0.5).to(cuda)
            ref = L.run_nhwc(ref, n, dt, osc, post)
            got = L.run_nhwc(got, n, dt, osc, post, trim=T)
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all() and ref.float().abs().max() > 0
    assert torch.equal(got, ref)
