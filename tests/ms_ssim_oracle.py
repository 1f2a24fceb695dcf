"""MS-SSIM in fp64 torch on the CPU: the reference the HIP kernels (ic2_ms_ssim_fwd / ic2_ms_ssim_bwd) are held to.

Definition (Wang, Simoncelli, Bovik 2003, as the common implementations evaluate it).  For NCHW batches X, Y with data
range L, per image and channel: window g[i] = exp(-(i-5)^2 / (2 * 1.5^2)), i = 0..10, normalised, applied separably with
no padding; C1 = (0.01 L)^2, C2 = (0.03 L)^2; mu = g*X, sigma_x^2 = g*X^2 - mu_x^2, sigma_xy = g*XY - mu_x mu_y;
cs = (2 sigma_xy + C2) / (sigma_x^2 + sigma_y^2 + C2), ssim = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs.  Five
scales; between scales a 2 x 2 mean pool, stride 2, that pads an odd axis by one zero at both ends (the padding counts
in the divisor), so output i covers inputs 2i-1, 2i and the length is (s+1)/2.  Term t_s = spatial mean of cs at scales
0..3 and of ssim at scale 4; value = mean_c prod_s max(t_s, 0)^w_s, w = WEIGHTS.  Gradients come from fp64 autograd on
exactly this; where any of a channel's terms is <= 0 the channel's product is 0 and its gradient is DEFINED as 0
(autograd of clamp gives that too: the clamped factor is 0 and has zero slope).

Error bounds (u = 2^-24; the kernels work in f32 on values centred at L/2, v = X - L/2, which leaves the variances and
the covariance unchanged and the means shifted by L/2).

Forward.  A filtered image g*p is two chains of 11 fmaf: at most 22 u relative to g*|p|, plus 1 u for the product p
and 2 u for the rounded taps; a pooled level carries 3 u per pool relative to |v|, 12 u at level 4, and enters the
second moments quadratically (24 u).  So with
    mbar = g*|v|,   Sxx = g*v^2 + 2 |mu'_x| mbar_x,   Sxy = g*|v_x v_y| + 2 max(|mu'_x| mbar_y, |mu'_y| mbar_x),
    M_N = 2 Sxy + C2,   M_D = Sxx + Syy + C2,   D = sigma_x^2 + sigma_y^2 + C2,
the numerator and the denominator of cs carry at most K u M_N and K u M_D, and cs itself
    A_cs = (M_N + |cs| M_D) / D                                     (per position, then averaged: A of the term)
with K <= 24 (levels) + 25 (second moment) + 2 * 24 (the square of a mean, both factors) + 3 (sums, division) = 100 in
the worst case where every rounding has the same sign.  The luminance factor has no cancellation (relative error
about 30 u of itself, its means being 22 u chains plus the centre), so A_ssim = |l| A_cs + |ssim|.  K_FWD_DERIVED = 100.
Roundings are not aligned and the term is a mean over >= 1 (121 windows' worth of pixels) .. 60 000 positions, so the
measured ratio is far below that; see tests/test_gpu_ms_ssim.py for measured and bar.

Backward.  The kernel recomputes the filtered images, forms the adjoint maps
    C = 2 / D,  B = -cs / D,  A_x = 2 (cs mu'_x - mu'_y) / D   (last scale: times / plus the luminance factor's parts),
scales them by gterms / positions, applies the transposed filter and combines g_x = A_x + 2 v_x B + v_y C, adds a
quarter of the coarser level's gradient, and halves at level 0.  ``grad_bound`` evaluates the same chain on error
magnitudes: each quantity q carries e_q = |q| + sum |dq/dp| e_p over its operands p (first-order propagation, the
project's B construction extended by the amplification through 1/D and cs), filtered by the same transposed window
and combined with |v_x|, |v_y|; the coarser level's bound enters with its quarter.  Every rounding error of a correctly
indexed kernel is K u times one term of that sum, K <= K_FWD_DERIVED + 24 (transposed filter) + 6 (scale, combination,
pool adjoint, halving) = 130 = K_BWD_DERIVED in the aligned worst case.

Case table (test_gpu_ms_ssim.py; values on the shapes used there, fp64):
    noisy        b = a + 0.05 randn on uniform a                      value ~ 0.9968, every term >= 0.996
    smooth       six random low-frequency sinusoids; b = 0.9 a + 0.04 randn + 0.03   value 0.989-0.990, terms >= 0.90
    independent  independent uniform images                           scale-0 term within +-0.05 of zero: terms only
    negated      b = -a on the smooth image                           terms down to -0.97; value 0, gradient 0
    clamped      values beyond [-1, 1]                                metric mode only
    identical    b = a                                                every term exactly 1.0
test_ms_ssim_oracle_host.py asserts that noisy and smooth keep every reference term above 0.5, so the value and
gradient bars never rest on an ill-conditioned power."""
import functools
import math

import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
TAPS, LEVELS = 11, 5
MIN_SIDE = (TAPS - 1) * 2 ** (LEVELS - 1) + 1
U = 2.0 ** -24
K_FWD_DERIVED = 100.0
K_BWD_DERIVED = 130.0


def window(dtype=torch.float64):
    i = torch.arange(TAPS, dtype=torch.float64)
    g = torch.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def gfilt(x, g=None):
    """Separable valid filter, rows then columns, of [P, 1, h, w]."""
    g = window(x.dtype) if g is None else g
    return F.conv2d(F.conv2d(x, g.view(1, 1, 1, TAPS)), g.view(1, 1, TAPS, 1))


def gfilt_t(x, g=None):
    """The transposed (full) filter: [P, 1, h-10, w-10] -> [P, 1, h, w]."""
    g = window(x.dtype) if g is None else g
    return F.conv_transpose2d(F.conv_transpose2d(x, g.view(1, 1, TAPS, 1)), g.view(1, 1, 1, TAPS))


def pool(x):
    h, w = x.shape[-2:]
    return F.avg_pool2d(F.pad(x, (w % 2, w % 2, h % 2, h % 2)), 2)


def pool_t(g, h, w):
    """Adjoint of ``pool`` for an input of h x w: a quarter of the covering cell's gradient."""
    up = g.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1) * 0.25
    return up[..., h % 2:h % 2 + h, w % 2:w % 2 + w]


def to_uint8(x):
    """The reference's conversion trunc(clamp(x*0.5+0.5, 0, 1)*255) in float32, as float64 integers."""
    return ((x.detach().float() * 0.5 + 0.5).clamp(0, 1) * 255).to(torch.uint8).double()


def loss_images(x):
    return x.double() * 0.5 + 0.5


def _moments(x, y):
    return gfilt(x), gfilt(y), gfilt(x * x), gfilt(y * y), gfilt(x * y)


def scale_maps(x, y, L):
    """cs and luminance maps of [P, 1, h, w] planes."""
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mx, my, exx, eyy, exy = _moments(x, y)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    lum = (2 * mx * my + c1) / (mx * mx + my * my + c1)
    return cs, lum


def terms_of(X, Y, L):
    """[N, C, H, W] images (any float dtype; fp64 for the reference) -> terms [N, C, 5]."""
    n, c, h, w = X.shape
    if min(h, w) < MIN_SIDE:
        raise ValueError(f"the smaller side must exceed {MIN_SIDE - 1}, got {h} x {w}")
    x, y = X.reshape(n * c, 1, h, w), Y.reshape(n * c, 1, h, w)
    out = []
    for s in range(LEVELS):
        cs, lum = scale_maps(x, y, L)
        out.append((cs * lum if s == LEVELS - 1 else cs).mean(dim=(1, 2, 3)))
        if s < LEVELS - 1:
            x, y = pool(x), pool(y)
    return torch.stack(out, dim=1).reshape(n, c, LEVELS)


def value_of(terms):
    w = torch.tensor(WEIGHTS, dtype=terms.dtype)
    return (terms.clamp_min(0) ** w).prod(dim=2).mean(dim=1)


def metric_terms(a, b):
    """Metric mode: the uint8 images with L = 255."""
    return terms_of(to_uint8(a), to_uint8(b), 255.0)


def loss_terms(a, b):
    """Loss mode: x*0.5+0.5 unclamped with L = 1."""
    return terms_of(loss_images(a), loss_images(b), 1.0)


def loss_and_grads(a, b, upstream):
    """1 - value per image [N] (fp64), and d (sum_n upstream[n] * loss[n]) / d a, / d b by fp64 autograd."""
    a64 = a.double().clone().requires_grad_(True)
    b64 = b.double().clone().requires_grad_(True)
    terms = terms_of(a64 * 0.5 + 0.5, b64 * 0.5 + 0.5, 1.0)
    loss = 1.0 - value_of(terms)
    ga, gb = torch.autograd.grad((loss * upstream.double()).sum(), (a64, b64))
    return loss.detach(), terms.detach(), ga, gb


# ------------------------------------------------------------------------------------------------ error magnitudes
def _point_magnitudes(x, y, L):
    """Per map position of centred planes x, y [P, 1, h, w]: the quantities of the forward and their first-order error
    magnitudes (module docstring).  Returns a dict of [P, 1, h-10, w-10] maps."""
    c1, c2, cen = (0.01 * L) ** 2, (0.03 * L) ** 2, 0.5 * L
    mx, my, exx, eyy, exy = _moments(x, y)
    bx, by, bxy = gfilt(x.abs()), gfilt(y.abs()), gfilt((x * y).abs())
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    D = sxx + syy + c2
    cs = (2 * sxy + c2) / D
    Sxx, Syy = exx + 2 * mx.abs() * bx, eyy + 2 * my.abs() * by
    Sxy = bxy + 2 * torch.maximum(mx.abs() * by, my.abs() * bx)
    M_N, M_D = 2 * Sxy + c2, Sxx + Syy + c2
    e_cs = (M_N + cs.abs() * M_D) / D
    ux, uy = mx + cen, my + cen
    Dl = ux * ux + uy * uy + c1
    lum = (2 * ux * uy + c1) / Dl
    return dict(mx=mx, my=my, bx=bx, by=by, D=D, cs=cs, M_D=M_D, e_cs=e_cs, ux=ux, uy=uy, Dl=Dl, lum=lum, c1=c1)


def forward_amplification(X, Y, L):
    """A [N, C, 5]: the per-term amplification of u in the forward (module docstring)."""
    n, c, h, w = X.shape
    x, y = (X - 0.5 * L).reshape(n * c, 1, h, w), (Y - 0.5 * L).reshape(n * c, 1, h, w)
    out = []
    for s in range(LEVELS):
        q = _point_magnitudes(x, y, L)
        a = q["e_cs"]
        if s == LEVELS - 1:
            a = q["lum"].abs() * a + (q["lum"] * q["cs"]).abs()
        out.append(a.mean(dim=(1, 2, 3)))
        if s < LEVELS - 1:
            x, y = pool(x + 0.5 * L) - 0.5 * L, pool(y + 0.5 * L) - 0.5 * L
    return torch.stack(out, dim=1).reshape(n, c, LEVELS)


def grad_bound(a, b, gterms):
    """G_a, G_b [N, C, H, W]: the backward chain on error magnitudes for loss mode (L = 1), given d L / d terms
    [N, C, 5] (module docstring).  A correctly indexed f32 kernel is within K u G of the fp64 gradient."""
    n, c, h, w = a.shape
    L = 1.0
    x = (a.double() * 0.5).reshape(n * c, 1, h, w)
    y = (b.double() * 0.5).reshape(n * c, 1, h, w)
    levels = []
    for s in range(LEVELS):
        levels.append((x, y))
        if s < LEVELS - 1:
            x, y = pool(x + 0.5) - 0.5, pool(y + 0.5) - 0.5
    Gx = Gy = None
    for s in reversed(range(LEVELS)):
        x, y = levels[s]
        q = _point_magnitudes(x, y, L)
        mx, my, bx, by, D, cs, e_cs = q["mx"], q["my"], q["bx"], q["by"], q["D"], q["cs"], q["e_cs"]
        inv_d, e_inv_d = 1 / D, q["M_D"] / (D * D)
        Ax, Ay = 2 * inv_d * (cs * mx - my), 2 * inv_d * (cs * my - mx)
        e_Ax = 2 * (e_inv_d * (cs * mx - my).abs() + inv_d * (e_cs * mx.abs() + cs.abs() * bx + by)) + Ax.abs()
        e_Ay = 2 * (e_inv_d * (cs * my - mx).abs() + inv_d * (e_cs * my.abs() + cs.abs() * by + bx)) + Ay.abs()
        B, C = -cs * inv_d, 2 * inv_d
        e_B, e_C = e_cs * inv_d + cs.abs() * e_inv_d + B.abs(), 2 * e_inv_d + C.abs()
        if s == LEVELS - 1:
            ux, uy, Dl, lum, c1 = q["ux"], q["uy"], q["Dl"], q["lum"], q["c1"]
            e_ux, e_uy = bx + ux.abs(), by + uy.abs()
            e_Nl = 2 * (ux.abs() * e_uy + uy.abs() * e_ux) + (2 * ux * uy + c1).abs()
            e_Dl = 2 * (ux.abs() * e_ux + uy.abs() * e_uy) + Dl
            e_l = (e_Nl + lum.abs() * e_Dl) / Dl
            inv_dl, e_inv_dl = 1 / Dl, e_Dl / (Dl * Dl)
            dlx, dly = 2 * inv_dl * (uy - lum * ux), 2 * inv_dl * (ux - lum * uy)
            e_dlx = 2 * (e_inv_dl * (uy - lum * ux).abs() + inv_dl * (e_uy + e_l * ux.abs() + lum.abs() * e_ux)) + dlx.abs()
            e_dly = 2 * (e_inv_dl * (ux - lum * uy).abs() + inv_dl * (e_ux + e_l * uy.abs() + lum.abs() * e_uy)) + dly.abs()
            e_Ax = e_cs * dlx.abs() + cs.abs() * e_dlx + e_l * Ax.abs() + lum.abs() * e_Ax
            e_Ay = e_cs * dly.abs() + cs.abs() * e_dly + e_l * Ay.abs() + lum.abs() * e_Ay
            e_B, e_C = e_l * B.abs() + lum.abs() * e_B, e_l * C.abs() + lum.abs() * e_C
        hs, ws_ = x.shape[-2:]
        sc = (gterms.double().reshape(n * c, LEVELS)[:, s].abs() / ((hs - 10) * (ws_ - 10))).view(-1, 1, 1, 1)
        tB, tC = gfilt_t(sc * e_B), gfilt_t(sc * e_C)
        gx = gfilt_t(sc * e_Ax) + 2 * x.abs() * tB + y.abs() * tC
        gy = gfilt_t(sc * e_Ay) + 2 * y.abs() * tB + x.abs() * tC
        if Gx is not None:
            gx, gy = gx + pool_t(Gx, hs, ws_), gy + pool_t(Gy, hs, ws_)
        Gx, Gy = gx, gy
    return (0.5 * Gx).reshape(n, c, h, w), (0.5 * Gy).reshape(n, c, h, w)


def gterms_of(terms, upstream):
    """d (sum_n upstream[n] * (1 - value[n])) / d terms, with the zero-gradient convention."""
    t = terms.detach().double().clone().requires_grad_(True)
    ((1.0 - value_of(t)) * upstream.double()).sum().backward()
    return t.grad


# ------------------------------------------------------------------------------------------------ the case table
TILE = (32, 32)     # metrics.MS_SSIM_TILE (test_ms_ssim_host.py holds the two equal)
SHAPES = [(2, 3, 161, 161), (1, 3, 176, 161), (1, 1, 161, 200), (1, 3, 163, 189), (2, 3, 256, 256)]


def tile_shapes(tile=TILE):
    """Three shapes whose scale-0 map extent (side - 10) is one short of, equal to, and one past a whole number of
    tiles on each axis (5 tiles of rows and of columns at the smallest legal multiple past 151 positions)."""
    ty, tx = tile
    ny, nx = math.ceil(151 / ty), math.ceil(151 / tx)
    return [(1, 1, ny * ty + 10 + d, nx * tx + 10 + d) for d in (-1, 0, 1)]


KINDS = ("noisy", "smooth", "independent", "negated", "clamped")


def _smooth(shape, g):
    n, c, h, w = shape
    yy = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1)
    xx = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
    img = torch.zeros(n, c, h, w, dtype=torch.float64)
    for _ in range(6):
        fy = torch.rand(n, c, 1, 1, generator=g, dtype=torch.float64) * 0.06
        fx = torch.rand(n, c, 1, 1, generator=g, dtype=torch.float64) * 0.06
        ph = torch.rand(n, c, 1, 1, generator=g, dtype=torch.float64) * 2 * math.pi
        amp = torch.rand(n, c, 1, 1, generator=g, dtype=torch.float64) * 0.25 + 0.05
        img += amp * torch.sin(2 * math.pi * (fy * yy + fx * xx) + ph)
    return img.float()


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    """The (a, b) f32 CPU pair of a case; cached and never modified."""
    g = torch.Generator().manual_seed(1000 + sum(shape) + 7 * KINDS.index(kind))
    if kind == "noisy":
        a = torch.rand(shape, generator=g) * 2 - 1
        b = a + 0.05 * torch.randn(shape, generator=g)
    elif kind == "smooth":
        a = _smooth(shape, g)
        b = 0.9 * a + 0.04 * torch.randn(shape, generator=g) + 0.03
    elif kind == "independent":
        a, b = torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1
    elif kind == "negated":
        a = _smooth(shape, g)
        b = -a
    else:
        assert kind == "clamped"
        a, b = torch.rand(shape, generator=g) * 2.4 - 1.2, torch.rand(shape, generator=g) * 2.6 - 1.3
    return a.contiguous(), b.contiguous()


def upstream_of(n):
    """A non-uniform upstream gradient per image."""
    return torch.tensor([0.7 + 0.9 * i for i in range(n)], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, mode):
    """dict(terms, value, A) of a case in 'loss' or 'metric' mode (fp64, read-only)."""
    a, b = inputs(shape, kind)
    if mode == "metric":
        X, Y, L = to_uint8(a), to_uint8(b), 255.0
    else:
        X, Y, L = loss_images(a), loss_images(b), 1.0
    terms = terms_of(X, Y, L)
    return dict(terms=terms, value=value_of(terms), A=forward_amplification(X, Y, L))


@functools.lru_cache(maxsize=None)
def reference_grads(shape, kind):
    """dict(loss, terms, ga, gb, Ga, Gb) of a loss-mode case with ``upstream_of`` (fp64, read-only)."""
    a, b = inputs(shape, kind)
    up = upstream_of(shape[0])
    loss, terms, ga, gb = loss_and_grads(a, b, up)
    Ga, Gb = grad_bound(a, b, gterms_of(terms, up))
    return dict(loss=loss, terms=terms, ga=ga, gb=gb, Ga=Ga, Gb=Gb)
