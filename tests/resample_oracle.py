"""NumPy restatement of Pillow's 8-bit resampler (Image.resize on "L" / "RGB" images): fixed-point coefficient tables
from doubles (math.sin, one rounding per written operation), then a horizontal and a vertical pass in int64 with the
uint8 clip between them.  test_resample_oracle_host.py pins it to PIL.Image.resize bit for bit; the native tables
(ic2_resample_coeffs) and kernels (ic2_resample_u8) are compared with it."""
import math

import numpy as np

BILINEAR, BICUBIC, LANCZOS = 0, 1, 2
FILTERS = {"bilinear": BILINEAR, "bicubic": BICUBIC, "lanczos": LANCZOS}
SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
PRECISION_BITS = 22

# (h, w, oh, ow): down, up, one axis unchanged, nothing to resize, 1-pixel outputs, 391 taps (a 65x downscale)
GEOMETRIES = [(61, 47, 16, 24), (129, 97, 24, 40), (70, 70, 33, 65), (16, 16, 32, 32), (7, 5, 8, 8), (32, 40, 32, 32),
              (40, 32, 32, 32), (32, 32, 32, 32), (37, 53, 1, 3), (520, 24, 8, 8), (24, 520, 8, 8), (300, 200, 32, 32)]


def make_image(h, w, c, kind, seed):
    """uint8 [h][w][c]: "noise", or "binary" (random 0 / 255: the overshoot of the cubic and Lanczos filters)."""
    rng = np.random.default_rng([seed, h, w, c, kind == "binary"])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, c)) * 255).astype(np.uint8)


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _filter(f, x):
    if f == BILINEAR:
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if f == BICUBIC:   # Keys, a = -0.5
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
        if x < 2.0:
            return (((x - 5.0) * x + 8.0) * x - 4.0) * a
        return 0.0
    if f == LANCZOS:
        return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0
    raise ValueError(f"unknown filter {f}")


def ksize(in_size, out_size, f):
    scale = in_size / out_size
    return int(math.ceil(SUPPORT[f] * max(scale, 1.0))) * 2 + 1


def coeffs(in_size, out_size, f):
    """(bounds [out][2] int32 = (xmin, taps), kk [out][ksize] int32, fixed point with 22 fraction bits)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[f] * fs
    ks = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros([out_size, 2], dtype=np.int32)
    kk = np.zeros([out_size, ks], dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5)) - xmin
        w = [_filter(f, (x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def identity(size):
    """The table of an axis that is not filtered: one tap of weight 1 on the pixel itself (exact)."""
    bounds = np.stack([np.arange(size), np.ones(size)], axis=1).astype(np.int32)
    return bounds, np.full([size, 1], 1 << PRECISION_BITS, dtype=np.int32)


def _pass(img, bounds, kk, first=0):
    """Filter axis 0 of img [in][...] (uint8) -> (uint8 [out][...], the accumulators >> 22 before the clip)."""
    out = np.zeros((bounds.shape[0],) + img.shape[1:], dtype=np.int64)
    src = img.astype(np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        k = kk[xx, :n].astype(np.int64).reshape((-1,) + (1,) * (img.ndim - 1))
        out[xx] = ((1 << (PRECISION_BITS - 1)) + (src[xmin - first:xmin - first + n] * k).sum(0)) >> PRECISION_BITS
    return np.clip(out, 0, 255).astype(np.uint8), out


def resize(img, size, f, return_preclip=False):
    """img uint8 [h][w] or [h][w][c] -> [oh][ow]([c]), size = (oh, ow): the horizontal pass over the source rows the
    vertical pass reads, then the vertical pass; an axis whose size does not change is not filtered."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8
    h, w = img.shape[:2]
    oh, ow = size
    pre = []
    by, ky = coeffs(h, oh, f) if oh != h else identity(h)
    y0, y1 = int(by[0, 0]), int(by[-1, 0] + by[-1, 1])
    cur = img[y0:y1]
    if ow != w:
        bx, kx = coeffs(w, ow, f)
        cur, p = _pass(np.swapaxes(cur, 0, 1), bx, kx)
        cur = np.swapaxes(cur, 0, 1)
        pre.append(np.swapaxes(p, 0, 1))
    if oh != h:
        cur, p = _pass(cur, by, ky, first=y0)
        pre.append(p)
    cur = np.ascontiguousarray(cur)
    return (cur, pre) if return_preclip else cur


def lut(c, mean=0.5, std=0.5):
    """ToTensor + Normalize as a table [c][256] f32, in torch's own arithmetic."""
    import torch
    mean = [mean] * c if isinstance(mean, (int, float)) else list(mean)
    std = [std] * c if isinstance(std, (int, float)) else list(std)
    base = torch.arange(256).float().div(255)
    return torch.stack([base.sub(m).div(s) for m, s in zip(mean, std)]).contiguous()
