"""GPU: the fused uint8 PSNR + SSIM pass (ic2_uint8_quality) against the CPU restatement of skimage's
structural_similarity (tests/ssim_oracle.py, pinned in test_quality_host.py), and the evaluation record built on it.

Bars.  The squared error is an exact integer below 2^53 in any order: array_equal to ic2_uint8_sse.  Per-image SSIM
within 1e-10 absolute of the restatement: the window moments are exact integers, S takes about a dozen float64
roundings, and the worst amplification is the variance difference (ulp(65025) = 7e-12 over C2 = 58.5), so < 1e-12 per
window and no worse in the mean; the restatement itself is within 8e-16 of exact integer moments.  A single
mis-indexed pixel moves a small image's SSIM by more than 1e-4."""
import functools

import numpy as np
import pytest
import torch

import image_compression_2_amd as ic2
from image_compression_2_amd import metrics as icm

import ssim_oracle as so

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-10

# The kernel's tile is icm.QUALITY_TILE = 32 x 64 window origins (rows x columns) per workgroup.  With the default
# 7 x 7 window an image of (oy + 6) x (ox + 6) pixels has oy x ox origins: one origin short of a full tile in each
# direction, and one origin into a second tile row and a second tile column.
_OY, _OX = icm.QUALITY_TILE
TILE_SHAPES = [(1, 3, _OY - 1 + 6, _OX - 1 + 6), (1, 3, _OY + 1 + 6, _OX + 1 + 6)]
SHAPES = [(2, 3, 7, 7), (2, 3, 8, 11), (1, 1, 7, 64), (1, 3, 23, 70), (3, 3, 33, 65), (1, 3, 64, 64),
          (1, 3, 256, 256)] + TILE_SHAPES
# W % 4 == 0 (the float4 staging) with a second tile row and column whose halo the last tiles own
SHAPES_EXTRA = [(2, 3, 40, 72)]
KINDS = ["clamped", "noisy", "saturated"]


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    g = torch.Generator().manual_seed(sum(shape) + len(kind))
    if kind == "clamped":      # beyond [-1, 1] on one side: exercises the clamp; SSIM ~ 0, may be negative
        return torch.rand(shape, generator=g) * 2.4 - 1.2, torch.rand(shape, generator=g) * 2 - 1
    if kind == "noisy":        # SSIM ~ 0.997
        a = torch.rand(shape, generator=g) * 2 - 1
        return a, a + 0.05 * torch.randn(shape, generator=g)
    assert kind == "saturated"
    return torch.full(shape, 2.0), torch.full(shape, -2.0)


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, win):
    a, b = _inputs(shape, kind)
    ref = so.ssim_batch(a, b, win)
    ref.setflags(write=False)
    return ref


def _check(cuda, shape, kind, win):
    a, b = _inputs(shape, kind)
    ad, bd = a.to(cuda), b.to(cuda)
    sse, ssim = icm.uint8_quality(ad, bd, win_size=win)
    assert sse.dtype == torch.float64 and ssim.dtype == torch.float64
    assert sse.shape == (shape[0],) and ssim.shape == (shape[0],) and sse.device == ad.device
    ref = _reference(shape, kind, win)
    err = np.abs(ssim.cpu().numpy() - ref).max()
    print(f"shape {shape} {kind} win {win}: ssim {ssim.cpu().numpy()} max|err| {err:.3e}")
    assert np.array_equal(sse.cpu().numpy(), icm.uint8_sse(ad, bd).cpu().numpy())
    assert err <= SSIM_TOL, (shape, kind, win, ssim.cpu().numpy(), ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES + SHAPES_EXTRA, ids=lambda s: "x".join(map(str, s)))
def test_uint8_quality_matches_restatement(cuda, shape, kind):
    _check(cuda, shape, kind, 7)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("win", [3, 11])
def test_uint8_quality_window_sizes(cuda, win, kind):
    _check(cuda, (1, 3, 23, 70), kind, win)


def test_saturated_images_closed_form(cuda):
    """+2 against -2 is 255 against 0 everywhere: S = C1 / (255^2 + C1) = 9.9990001e-5 in every window."""
    a, b = _inputs((1, 3, 23, 70), "saturated")
    sse, ssim = icm.uint8_quality(a.to(cuda), b.to(cuda))
    assert sse.item() == 255.0 ** 2 * a.numel()
    assert abs(ssim.item() - so.C1 / (255.0 ** 2 + so.C1)) <= 1e-15


@pytest.mark.parametrize("shape", [(2, 3, 23, 70), (1, 3, 64, 64), (1, 3, 40, 72)], ids=lambda s: "x".join(map(str, s)))
def test_identical_images_give_exactly_one(cuda, shape):
    a = _inputs(shape, "clamped")[0].to(cuda)
    for win in (3, 7, 11):
        sse, ssim = icm.uint8_quality(a, a.clone(), win_size=win)
        assert sse.tolist() == [0.0] * shape[0]
        assert ssim.tolist() == [1.0] * shape[0]
    assert icm.ssim(a, a) == 1.0


@pytest.mark.parametrize("shape", [(3, 3, 33, 65), (3, 3, 40, 72)], ids=lambda s: "x".join(map(str, s)))
def test_images_of_a_batch_do_not_mix(cuda, shape):
    a, b = (t.to(cuda) for t in _inputs(shape, "noisy"))
    sse3, ssim3 = icm.uint8_quality(a, b)
    sse1, ssim1 = icm.uint8_quality(a[1:2].clone(), b[1:2].clone())
    assert sse3[1].item() == sse1[0].item()
    assert ssim3[1].item() == ssim1[0].item()   # bitwise: an image's partials and their order do not depend on N
    assert icm.ssim(a, b) == sum(ssim3.tolist()) / 3


def test_two_runs_are_bitwise_equal(cuda):
    a, b = (t.to(cuda) for t in _inputs((1, 3, 256, 256), "noisy"))
    r1, r2 = icm.uint8_quality(a, b), icm.uint8_quality(a, b)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


def test_strided_input_equals_its_contiguous_copy(cuda):
    g = torch.Generator().manual_seed(11)
    wide_a = (torch.rand(2, 5, 23, 70, generator=g) * 2 - 1).to(cuda)
    wide_b = (torch.rand(2, 5, 23, 70, generator=g) * 2 - 1).to(cuda)
    va, vb = wide_a[:, 1:4], wide_b[:, ::2]       # channel-sliced views
    assert not va.is_contiguous() and not vb.is_contiguous()
    r_view = icm.uint8_quality(va, vb)
    r_copy = icm.uint8_quality(va.contiguous(), vb.contiguous())
    assert torch.equal(r_view[0], r_copy[0]) and torch.equal(r_view[1], r_copy[1])
    assert np.abs(r_view[1].cpu().numpy() - so.ssim_batch(va.cpu(), vb.cpu())).max() <= SSIM_TOL


def test_invalid_window_raises(cuda):
    a = torch.zeros(1, 3, 8, 8, device=cuda)
    with pytest.raises(RuntimeError, match="win=4"):
        icm.uint8_quality(a, a, win_size=4)
    with pytest.raises(RuntimeError, match="win=11"):
        icm.uint8_quality(a, a, win_size=11)     # the window exceeds the 8 x 8 image


# ------------------------------------------------------------------ the evaluation record
RECORD_KEYS = {"original_size_bytes", "compressed_size_bytes", "compression_ratio", "bpp", "psnr_no_quant",
               "ssim_no_quant", "psnr_quantized", "ssim_quantized", "batch_psnr_no_quant", "batch_ssim_no_quant",
               "batch_psnr_quantized", "batch_ssim_quantized", "n_images"}


def test_evaluate_compression_record(cuda):
    torch.manual_seed(1)
    G = ic2.Generator(img_resolution=256).to(cuda).eval()
    torch.manual_seed(7)
    enc = ic2.HVAE_VGG_Encoder(img_resolution=64, channel_base=256, channel_max=32).to(cuda)
    comp = ic2.StyleGAN3Compressor(enc, G, training_resolution=64)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    bits = 8
    torch.manual_seed(3)        # the encoder draws from the global generators (reparameterisation, fc1)
    rec = ic2.evaluate_compression(comp, x, quantization_bits=bits)
    assert set(rec) == RECORD_KEYS
    # hvae_training.py:354-359, per image: 16 x 512 W+ values
    comp_bytes = 16 * 512 * (bits / 8)
    orig_bytes = 3 * 64 * 64 * 4
    assert rec["compressed_size_bytes"] == comp_bytes and rec["original_size_bytes"] == orig_bytes
    assert rec["compression_ratio"] == orig_bytes / comp_bytes
    assert rec["bpp"] == comp_bytes * 8 / (256 * 256)
    # score the quantized branch independently.  compress() encodes the means, but the encoder redraws the fine
    # projector's fc1 on every call (as the reference does), so replay the record's call sequence from the same seed
    torch.manual_seed(3)
    with torch.no_grad():
        comp(x)
        rq = ic2.resize_bilinear(comp.decompress(comp.compress(x, bits)), (64, 64))
    sse = icm.uint8_sse(rq, x).cpu().tolist()
    ref_ssim = so.ssim_batch(rq.cpu(), x.cpu())
    for n in range(2):
        assert rec["psnr_quantized"][n] == pytest.approx(icm.psnr_from_sums(sse[n], 3 * 64 * 64), abs=1e-9)
        assert abs(rec["ssim_quantized"][n] - ref_ssim[n]) <= SSIM_TOL
    assert rec["batch_psnr_quantized"] == pytest.approx(icm.psnr_from_sums(sum(sse), 2 * 3 * 64 * 64), abs=1e-9)
    assert rec["batch_ssim_quantized"] == pytest.approx(ref_ssim.mean(), abs=SSIM_TOL)
    assert len(rec["psnr_no_quant"]) == len(rec["ssim_no_quant"]) == 2 and rec["n_images"] == 2
    assert all(np.isfinite(v) and -1.0 <= v <= 1.0 for v in rec["ssim_no_quant"])
    # a single process reduces to itself
    torch.manual_seed(3)
    assert ic2.evaluate_compression(comp, x, quantization_bits=bits, reduce=True) == rec
