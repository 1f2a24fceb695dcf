"""PSNR and SSIM exactly as the reference evaluates them (hvae_training.py:368-395): uint8 conversion
trunc(clamp(x*0.5+0.5, 0, 1)*255), then 10*log10(255^2 / MSE) in float64 (skimage 0.18 definition) and
skimage's structural_similarity(channel_axis=2, data_range=255) defaults: uniform 7x7 window, sample covariance,
K1 = 0.01, K2 = 0.03, the mean of the SSIM map over the windows that lie fully inside the image, then over channels.
The per-image squared-error sums run in one HIP kernel (ic2_uint8_sse); ic2_uint8_quality gives them together with
the per-(image, channel) SSIM-map sums in one pass over both images.  The log, the division by the window count and
the channel mean are host arithmetic.  ``evaluate_compression`` restates the record of the reference's
``test_compression`` (hvae_training.py:342-424) for a batch."""
from __future__ import annotations

import math

import torch

from . import _native as nv

# window origins (rows, columns) one workgroup of ic2_uint8_quality owns: QT_OY x QT_OX of csrc/metrics.hip
QUALITY_TILE = (32, 64)


def uint8_sse(a, b):
    """Per-image sum of squared uint8 differences -> float64 [N] (device)."""
    a = a.to(torch.float32).contiguous()
    b = b.to(torch.float32).contiguous()
    nv.require_gpu(a, b)
    assert a.shape == b.shape
    n = a.shape[0]
    out = torch.empty(n, dtype=torch.float64, device=a.device)
    scratch = torch.empty(int(nv.query("ic2_uint8_sse_scratch_doubles", n)), dtype=torch.float64, device=a.device)
    nv.call("ic2_uint8_sse", nv.ptr(a), nv.ptr(b), n, a[0].numel(), nv.ptr(out), nv.ptr(scratch), nv.stream_of(a))
    return out


def psnr_from_sums(sse_total, n_values):
    mse = float(sse_total) / float(n_values)
    return float("inf") if mse == 0 else 10.0 * math.log10(255.0 ** 2 / mse)


def psnr(a, b):
    sse = uint8_sse(a, b)
    return psnr_from_sums(sse.sum().item(), a.numel())


def n_windows(h, w, win_size=7):
    """Windows of win_size x win_size that lie fully inside an h x w image (what skimage's cropped mean covers)."""
    return (h - win_size + 1) * (w - win_size + 1)


def _uint8_quality_sums(a, b, win_size):
    a = a.to(torch.float32).contiguous()
    b = b.to(torch.float32).contiguous()
    nv.require_gpu(a, b)
    assert a.shape == b.shape and a.dim() == 4, (a.shape, b.shape)
    n, c, h, w = a.shape
    win = int(win_size)
    sse = torch.empty(n, dtype=torch.float64, device=a.device)
    ssim_sum = torch.empty([n, c], dtype=torch.float64, device=a.device)
    n_scratch = int(nv.query("ic2_uint8_quality_scratch_doubles", n, c, h, w, win))
    scratch = torch.empty(max(n_scratch, 1), dtype=torch.float64, device=a.device)
    # an invalid shape or window (scratch query 0) is reported by the entry point's own validation, before any launch
    nv.call("ic2_uint8_quality", nv.ptr(a), nv.ptr(b), n, c, h, w, win, nv.ptr(sse), nv.ptr(ssim_sum), nv.ptr(scratch),
            nv.stream_of(a))
    return sse, ssim_sum


def uint8_quality(a, b, win_size=7):
    """One pass over two NCHW batches in nominal [-1, 1] -> (sse [N], ssim [N]), float64 on the device: the per-image
    uint8 squared error (as ``uint8_sse``) and the per-image SSIM, the mean over channels of the mean SSIM map."""
    sse, ssim_sum = _uint8_quality_sums(a, b, win_size)
    # device tensors as divisors: a Python scalar divisor is applied on the device as a multiplication by its rounded
    # reciprocal, which would turn the exact 1.0 of identical images into 1 - 2^-52 for some window counts
    n_win = torch.full((), n_windows(a.shape[2], a.shape[3], int(win_size)), dtype=torch.float64, device=sse.device)
    n_ch = torch.full((), a.shape[1], dtype=torch.float64, device=sse.device)
    return sse, (ssim_sum / n_win).sum(dim=1) / n_ch


def ssim_from_sums(ssim_sum_total, n_window_values):
    """Mean SSIM from a sum of SSIM-map values and the number of values summed (windows x channels x images): the
    counterpart of ``psnr_from_sums`` for all-reduced sums."""
    return float(ssim_sum_total) / float(n_window_values)


def ssim(a, b, win_size=7):
    """Mean over the batch of the per-image SSIMs."""
    per_image = uint8_quality(a, b, win_size)[1].tolist()
    return sum(per_image) / len(per_image)


# layout of the all-reduced quality record (distributed.metric_vector with `extra`): the quantized reconstruction's
# squared error leads, as in the benchmark's metric vector
_Q_SSE_Q, _Q_NVAL, _Q_NIMG, _Q_SSIM_Q, _Q_NWIN, _Q_SSE_NQ, _Q_SSIM_NQ = range(7)


def quality_record(sse_no_quant, ssim_sum_no_quant, sse_quantized, ssim_sum_quantized, n_values, n_window_values,
                   n_images):
    """The float64 vector of sums one rank contributes (summed across ranks by ``distributed.allreduce_sum``):
    squared errors, SSIM-map sums and the counts they are taken over."""
    from . import distributed as icd
    return icd.metric_vector(sse_quantized, n_values, n_images,
                             extra=(ssim_sum_quantized, n_window_values, sse_no_quant, ssim_sum_no_quant))


def figures_from_record(vec):
    """Sums -> batch figures (pure host arithmetic): PSNR of the pooled MSE and mean SSIM, for the reconstruction
    without and with quantization."""
    v = [float(t) for t in vec]
    return {"n_images": int(v[_Q_NIMG]),
            "batch_psnr_no_quant": psnr_from_sums(v[_Q_SSE_NQ], v[_Q_NVAL]),
            "batch_ssim_no_quant": ssim_from_sums(v[_Q_SSIM_NQ], v[_Q_NWIN]),
            "batch_psnr_quantized": psnr_from_sums(v[_Q_SSE_Q], v[_Q_NVAL]),
            "batch_ssim_quantized": ssim_from_sums(v[_Q_SSIM_Q], v[_Q_NWIN])}


def evaluate_compression(compressor, x, quantization_bits=8, noise_mode="const", reduce=False, win_size=7):
    """The record of the reference's ``test_compression`` (hvae_training.py:342-424) for a batch ``x`` [N, C, H, W]:
    reconstruct without quantization, compress, decompress, and score both reconstructions against ``x``.

    Sizes are per image with the reference's arithmetic (:354-359): ``compressed_size_bytes`` = W+ values per image *
    bits / 8, ``original_size_bytes`` = image values * 4, ``bpp`` over ``generator.img_resolution`` squared.
    ``psnr_*`` / ``ssim_*`` are per-image lists (the reference scores one image at a time).  The ``batch_*`` figures
    come from the sums over the batch: the PSNR of the pooled MSE (as ``psnr``) and the mean SSIM.  With
    ``reduce=True`` those sums are all-reduced over the process group first, so every rank reports the figures of the
    global batch (``n_images`` counts it); the per-image lists stay local."""
    from . import distributed as icd
    from .stylegan3_hvae_full import resize_bilinear
    with torch.no_grad():
        recon, w_plus = compressor(x, noise_mode=noise_mode)
        w_quantized = compressor.compress(x, quantization_bits)
        recon_quantized = compressor.decompress(w_quantized, noise_mode=noise_mode)
        n, c, h, w = x.shape
        sums = []
        for img in (recon, recon_quantized):
            if img.shape[2:] != x.shape[2:]:
                img = resize_bilinear(img, (h, w))
            sse, ssim_sum = _uint8_quality_sums(img, x, win_size)
            sums.append((sse.cpu(), ssim_sum.cpu()))
    n_win = n_windows(h, w, int(win_size))
    per_image_values = c * h * w
    res = compressor.generator.img_resolution
    compressed_size_bytes = (w_plus.numel() // n) * (quantization_bits / 8)
    original_size_bytes = per_image_values * 4
    out = {"original_size_bytes": original_size_bytes,
           "compressed_size_bytes": compressed_size_bytes,
           "compression_ratio": original_size_bytes / compressed_size_bytes,
           "bpp": compressed_size_bytes * 8 / (res * res)}
    for name, (sse, ssim_sum) in zip(("no_quant", "quantized"), sums):
        out["psnr_" + name] = [psnr_from_sums(s, per_image_values) for s in sse.tolist()]
        out["ssim_" + name] = [sum(s / n_win for s in row) / c for row in ssim_sum.tolist()]
    (sse_nq, ssim_nq), (sse_q, ssim_q) = sums
    vec = quality_record(sse_nq.sum().item(), ssim_nq.sum().item(), sse_q.sum().item(), ssim_q.sum().item(),
                         n * per_image_values, n * c * n_win, n)
    if reduce:
        vec = icd.allreduce_sum(vec, device=x.device)
    out.update(figures_from_record(vec))
    return out
