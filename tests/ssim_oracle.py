"""TEST INFRASTRUCTURE -- skimage's ``structural_similarity`` restated on the CPU, for the SSIM tests.

The reference scores its reconstructions with ``structural_similarity(a, b, channel_axis=2, data_range=255)`` on
uint8 HWC images (hvae_training.py:382-395).  skimage is not a dependency of this project, so its defaults are
restated here step by step: float64 images, ``scipy.ndimage.uniform_filter`` of size 7, sample covariance,
K1 = 0.01, K2 = 0.03, ``crop(S, (win_size - 1) // 2).mean()`` per channel, then the mean over channels.
``ssim_bruteforce`` is an independent formulation (exact integer window moments) that pins the restatement.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
from scipy.ndimage import uniform_filter

from oracle import metrics as om

K1, K2 = 0.01, 0.03
DATA_RANGE = 255
C1 = (K1 * DATA_RANGE) ** 2
C2 = (K2 * DATA_RANGE) ** 2


def _ssim_plane(im1, im2, win_size):
    """One channel (2-D uint8): the single-channel branch of structural_similarity."""
    if im1.shape[0] < win_size or im1.shape[1] < win_size:
        raise ValueError("win_size exceeds image extent")
    if win_size % 2 != 1:
        raise ValueError("Window size must be odd.")
    im1 = im1.astype(np.float64)
    im2 = im2.astype(np.float64)
    NP = win_size ** im1.ndim
    cov_norm = NP / (NP - 1)  # sample covariance
    ux = uniform_filter(im1, size=win_size)
    uy = uniform_filter(im2, size=win_size)
    uxx = uniform_filter(im1 * im1, size=win_size)
    uyy = uniform_filter(im2 * im2, size=win_size)
    uxy = uniform_filter(im1 * im2, size=win_size)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    A1, A2, B1, B2 = (2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2)
    S = (A1 * A2) / (B1 * B2)
    pad = (win_size - 1) // 2
    return S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64)


def ssim_uint8(im1, im2, win_size=7):
    """structural_similarity(im1, im2, channel_axis=2, data_range=255, win_size=win_size) of HWC uint8 images."""
    assert im1.dtype == np.uint8 and im2.dtype == np.uint8 and im1.shape == im2.shape and im1.ndim == 3
    nch = im1.shape[2]
    mssim = np.empty(nch, dtype=np.float64)
    for ch in range(nch):
        mssim[ch] = _ssim_plane(im1[..., ch], im2[..., ch], win_size)
    return float(mssim.mean())


def ssim_bruteforce(im1, im2, win_size=7):
    """The same number from exact integer moments of every fully-inside window (no filter, no border)."""
    nch = im1.shape[2]
    NP = win_size * win_size
    cov_norm = NP / (NP - 1)
    out = np.empty(nch, dtype=np.float64)
    for ch in range(nch):
        x = sliding_window_view(im1[..., ch].astype(np.int64), (win_size, win_size))
        y = sliding_window_view(im2[..., ch].astype(np.int64), (win_size, win_size))
        sx, sy = x.sum((2, 3)), y.sum((2, 3))
        sxx, syy, sxy = (x * x).sum((2, 3)), (y * y).sum((2, 3)), (x * y).sum((2, 3))
        ux, uy = sx / NP, sy / NP
        vx = cov_norm * (sxx / NP - ux * ux)
        vy = cov_norm * (syy / NP - uy * uy)
        vxy = cov_norm * (sxy / NP - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        out[ch] = S.mean(dtype=np.float64)
    return float(out.mean())


def ssim_batch(a, b, win_size=7):
    """Per-image SSIM of two NCHW float batches in nominal [-1, 1] -> float64 [N] (uint8 as the reference converts)."""
    ua, ub = om.to_uint8(a), om.to_uint8(b)
    return np.array([ssim_uint8(ua[i], ub[i], win_size) for i in range(ua.shape[0])], dtype=np.float64)
