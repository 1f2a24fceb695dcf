"""PSNR and SSIM exactly as the reference evaluates them (hvae_training.py:368-395): uint8 conversion
trunc(clamp(x*0.5+0.5, 0, 1)*255), then 10*log10(255^2 / MSE) in float64 (skimage 0.18 definition) and
skimage's structural_similarity(channel_axis=2, data_range=255) defaults: uniform 7x7 window, sample covariance,
K1 = 0.01, K2 = 0.03, the mean of the SSIM map over the windows that lie fully inside the image, then over channels.
The per-image squared-error sums run in one HIP kernel (ic2_uint8_sse); ic2_uint8_quality gives them together with
the per-(image, channel) SSIM-map sums in one pass over both images.  The log, the division by the window count and
the channel mean are host arithmetic.  ``evaluate_compression`` restates the record of the reference's
``test_compression`` (hvae_training.py:342-424) for a batch.

MS-SSIM, the third figure the reference's README reports, runs on the same footing (ic2_ms_ssim_fwd / ic2_ms_ssim_bwd,
csrc/msssim.hip): ``ms_ssim_terms`` gives the per-(image, channel, scale) terms, ``uint8_ms_ssim`` / ``ms_ssim`` the
evaluation figure on the uint8 images, and ``ms_ssim_loss`` / ``MSSSIMLoss`` the differentiable 1 - MS-SSIM with a HIP
backward: the perceptual training term that needs no pretrained weights (``training.train_step(percep=...)``)."""
from __future__ import annotations

import math

import torch

from . import _native as nv

# window origins (rows, columns) one workgroup of ic2_uint8_quality owns: QT_OY x QT_OX of csrc/metrics.hip
QUALITY_TILE = (32, 64)
# map positions (rows, columns) one workgroup of ic2_ms_ssim_fwd owns per scale: MT_Y x MT_X of csrc/msssim.hip
MS_SSIM_TILE = (32, 32)
# the exponents of the five scales (Wang, Simoncelli, Bovik 2003), finest first
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
# the smaller image side must exceed (11 - 1) * 2^4: the fifth scale holds at least one 11 x 11 window
MS_SSIM_MIN_SIDE = 161
_MS_LOSS, _MS_METRIC = 0, 1    # ic2ops.h IC2_MS_SSIM_LOSS / IC2_MS_SSIM_METRIC


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


def _ms_refuse_capture(t):
    """The Python layer of MS-SSIM is not capturable: it forms the value and d L / d terms with float64 torch ops and,
    for the loss, runs its backward from the autograd engine's thread, and a capture of exactly that ended in a host
    segmentation fault inside the capture's end on the MI355X whose cause is not established.  Refuse before anything
    is launched instead.  ic2_ms_ssim_fwd / ic2_ms_ssim_bwd on caller-owned buffers are capturable (they neither
    allocate nor synchronise; tests/test_gpu_ms_ssim.py replays them from a graph bit for bit)."""
    if t.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("ms_ssim: the Python layer (ms_ssim_terms, uint8_ms_ssim, ms_ssim, ms_ssim_loss, MSSSIMLoss) "
                           "refuses to run inside a graph capture; run it outside the capture, or capture "
                           "ic2_ms_ssim_fwd / ic2_ms_ssim_bwd on preallocated buffers (metrics._ms_refuse_capture)")


def _ms_ssim_check(a, b):
    nv.require_gpu(a, b)
    _ms_refuse_capture(a)
    if a.shape != b.shape or a.dim() != 4:
        raise ValueError(f"ms_ssim: expected two NCHW batches of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    n, c, h, w = a.shape
    if min(n, c) < 1 or min(h, w) < MS_SSIM_MIN_SIDE:
        raise ValueError(f"ms_ssim: shape {tuple(a.shape)}: the batch must not be empty and the smaller image side "
                         f"must exceed (11 - 1) * 2^4 = {MS_SSIM_MIN_SIDE - 1} for five scales")
    return n, c, h, w


def _ms_ssim_forward(a, b, mode):
    """a, b: contiguous f32 NCHW on the device -> (terms f64 [N, C, 5], the forward workspace)."""
    n, c, h, w = _ms_ssim_check(a, b)
    terms = torch.empty([n, c, 5], dtype=torch.float64, device=a.device)
    # float64 storage: the workspace starts with the f64 partials (8-byte aligned)
    ws = torch.empty((int(nv.query("ic2_ms_ssim_ws_floats", n, c, h, w)) + 1) // 2, dtype=torch.float64,
                     device=a.device)
    nv.call("ic2_ms_ssim_fwd", nv.ptr(a), nv.ptr(b), mode, n, c, h, w, nv.ptr(terms), nv.ptr(ws), nv.stream_of(a))
    return terms, ws


_ms_weight_cache = {}


def _ms_weights(device):
    """MS_SSIM_WEIGHTS as a float64 device tensor, uploaded once per device (no host-to-device copy per call)."""
    key = (device.type, device.index)
    if key not in _ms_weight_cache:
        _ms_weight_cache[key] = torch.tensor(MS_SSIM_WEIGHTS, dtype=torch.float64, device=device)
    return _ms_weight_cache[key]


def _ms_ssim_value(terms):
    """terms f64 [N, C, 5] -> per-image value f64 [N]: mean over channels of prod_s max(t_s, 0) ** w_s."""
    wts = _ms_weights(terms.device)
    return (terms.clamp_min(0) ** wts).prod(dim=2).mean(dim=1)


def ms_ssim_terms(a, b, uint8=True):
    """The five MS-SSIM terms per (image, channel) of two NCHW batches in nominal [-1, 1] -> float64 [N, C, 5] on the
    device: the spatial mean of cs at scales 0..3 and of ssim at scale 4 (11-tap Gaussian window, sigma 1.5, no
    padding; 2 x 2 mean pool between scales, an odd axis padded by one zero at both ends).  ``uint8=True`` scores the
    reference's uint8 images with data range 255 (the metric); ``uint8=False`` scores x*0.5+0.5 unclamped with data
    range 1 (what ``ms_ssim_loss`` differentiates).  Shapes whose smaller side is below 161 raise ValueError.  Not
    capturable in a graph: inside a capture this raises RuntimeError (``_ms_refuse_capture``)."""
    _ms_refuse_capture(a)
    a = a.to(torch.float32).contiguous()
    b = b.to(torch.float32).contiguous()
    return _ms_ssim_forward(a, b, _MS_METRIC if uint8 else _MS_LOSS)[0]


def uint8_ms_ssim(a, b):
    """Per-image MS-SSIM of the uint8 images -> float64 [N] on the device: mean over channels of
    prod_s max(t_s, 0) ** w_s with the weights ``MS_SSIM_WEIGHTS``."""
    return _ms_ssim_value(ms_ssim_terms(a, b, uint8=True))


def ms_ssim(a, b):
    """Mean over the batch of the per-image MS-SSIMs (the counterpart of ``ssim``)."""
    per_image = uint8_ms_ssim(a, b).tolist()
    return sum(per_image) / len(per_image)


class _MSSSIMLossBackwardFn(torch.autograd.Function):
    """ic2_ms_ssim_bwd as a graph node of its own: a second differentiation (create_graph=True) reaches a backward
    that refuses instead of silently treating the gradient as a constant."""

    @staticmethod
    def forward(ctx, grad_out, a, b, ws, terms, need_a, need_b):
        _ms_refuse_capture(a)
        n, c, h, w = a.shape
        wts = _ms_weights(terms.device)
        # d value_c / d t_s = w_s * value_c / t_s where all five terms are positive, 0 where any is not (the product
        # is 0 there and max(t, 0) ** w has no finite derivative at 0)
        alive = (terms > 0).all(dim=2, keepdim=True)
        safe = torch.where(alive, terms, torch.ones_like(terms))
        value_c = (safe ** wts).prod(dim=2, keepdim=True)
        upstream = (-grad_out.to(torch.float64) / c).view(n, 1, 1)
        gterms = torch.where(alive, upstream * wts * value_c / safe, torch.zeros_like(terms)).contiguous()
        ga = torch.empty_like(a) if need_a else None
        gb = torch.empty_like(b) if need_b else None
        ws_grad = torch.empty(max(int(nv.query("ic2_ms_ssim_bwd_ws_floats", n, c, h, w)), 1), dtype=torch.float32,
                              device=a.device)
        nv.call("ic2_ms_ssim_bwd", nv.ptr(a), nv.ptr(b), _MS_LOSS, nv.ptr(ws), nv.ptr(gterms), n, c, h, w, nv.ptr(ga),
                nv.ptr(gb), nv.ptr(ws_grad), nv.stream_of(a))
        return ga, gb

    @staticmethod
    def backward(ctx, *grads):
        raise nv.AutogradUnsupported("ms_ssim_loss: double backward (differentiating its gradient) is not implemented "
                                     "on the HIP path")


class _MSSSIMLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        terms, ws = _ms_ssim_forward(a, b, _MS_LOSS)
        ctx.save_for_backward(a, b, ws, terms)
        return (1.0 - _ms_ssim_value(terms)).to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        a, b, ws, terms = ctx.saved_tensors
        return _MSSSIMLossBackwardFn.apply(grad_out, a, b, ws, terms, ctx.needs_input_grad[0],
                                           ctx.needs_input_grad[1])


def ms_ssim_loss(a, b):
    """1 - MS-SSIM per image -> float32 [N], differentiable with respect to either or both inputs (HIP forward and
    backward).  a, b: NCHW in nominal [-1, 1]; the images scored are x*0.5+0.5, unclamped, with data range 1 (the
    metric's uint8 truncation has no gradient).  Only the gradients autograd asks for are computed.

    Gradient convention (a deviation from the plain chain rule): prod_s max(t_s, 0) ** w_s has no finite derivative
    at t_s = 0, so where any of a channel's five terms is <= 0 that channel's product is 0 and its gradient is defined
    as 0; everywhere else the gradient is the chain rule's.  Differentiating the backward again raises.

    Inputs of another dtype (the f16 reconstruction of the loss-scaled training step) are cast to float32 by torch, one
    elementwise pass over the image each way; the kernels read float32.

    Not capturable: called while the current stream is capturing a graph (a captured training step, for instance),
    forward or backward, this raises RuntimeError before anything is launched (``_ms_refuse_capture`` says why).  The
    two C entry points on caller-owned buffers are the capturable interface."""
    _ms_refuse_capture(a)
    a = a.to(torch.float32).contiguous()
    b = b.to(torch.float32).contiguous()
    _ms_ssim_check(a, b)
    if not (torch.is_grad_enabled() and (a.requires_grad or b.requires_grad)):
        return (1.0 - _ms_ssim_value(_ms_ssim_forward(a, b, _MS_LOSS)[0])).to(torch.float32)
    return _MSSSIMLossFn.apply(a, b)


class MSSSIMLoss(torch.nn.Module):
    """``ms_ssim_loss`` as the ``percep`` callable of ``training.train_step`` / ``train_step_gumbel``:
    ``MSSSIMLoss()(images, reconstructed)`` -> float32 [N].  No parameters, no pretrained weights.  Like
    ``ms_ssim_loss`` it refuses to run inside a graph capture (RuntimeError): a step that uses it is run eagerly."""

    def forward(self, images, reconstructed):
        return ms_ssim_loss(images, reconstructed)


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


def evaluate_compression(compressor, x, quantization_bits=8, noise_mode="const", reduce=False, win_size=7,
                         ms_ssim=False):
    """The record of the reference's ``test_compression`` (hvae_training.py:342-424) for a batch ``x`` [N, C, H, W]:
    reconstruct without quantization, compress, decompress, and score both reconstructions against ``x``.

    Sizes are per image with the reference's arithmetic (:354-359): ``compressed_size_bytes`` = W+ values per image *
    bits / 8, ``original_size_bytes`` = image values * 4, ``bpp`` over ``generator.img_resolution`` squared.
    ``psnr_*`` / ``ssim_*`` are per-image lists (the reference scores one image at a time).  The ``batch_*`` figures
    come from the sums over the batch: the PSNR of the pooled MSE (as ``psnr``) and the mean SSIM.  With
    ``reduce=True`` those sums are all-reduced over the process group first, so every rank reports the figures of the
    global batch (``n_images`` counts it); the per-image lists stay local.

    ``ms_ssim=True`` adds the third figure the reference's README reports: ``ms_ssim_no_quant`` / ``ms_ssim_quantized``
    (per-image lists, ``uint8_ms_ssim``) and ``batch_ms_ssim_*`` (the mean over the images; with ``reduce=True`` from
    the all-reduced sum and image count).  It needs images whose smaller side exceeds 160.  With the default the
    record is key for key what it was."""
    from . import distributed as icd
    from .stylegan3_hvae_full import resize_bilinear
    with torch.no_grad():
        recon, w_plus = compressor(x, noise_mode=noise_mode)
        w_quantized = compressor.compress(x, quantization_bits)
        recon_quantized = compressor.decompress(w_quantized, noise_mode=noise_mode)
        n, c, h, w = x.shape
        sums, ms_values = [], []
        for img in (recon, recon_quantized):
            if img.shape[2:] != x.shape[2:]:
                img = resize_bilinear(img, (h, w))
            sse, ssim_sum = _uint8_quality_sums(img, x, win_size)
            sums.append((sse.cpu(), ssim_sum.cpu()))
            if ms_ssim:
                ms_values.append(uint8_ms_ssim(img, x).cpu())
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
    if ms_ssim:
        ms_vec = torch.tensor([v.sum().item() for v in ms_values] + [float(n)], dtype=torch.float64)
        if reduce:
            ms_vec = icd.allreduce_sum(ms_vec, device=x.device)
        for i, name in enumerate(("no_quant", "quantized")):
            out["ms_ssim_" + name] = ms_values[i].tolist()
            out["batch_ms_ssim_" + name] = float(ms_vec[i]) / float(ms_vec[2])
    return out
