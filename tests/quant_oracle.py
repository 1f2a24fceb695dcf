"""Plain torch references for the latent quantizers of csrc/quant.hip: the operations, not the kernels.

Decisions are exact f32 arithmetic and get an f32 CPU reference that the kernels must match bit for bit:

  uniform(w, bits) -> (q, idx)   (w + 1) * 0.5, round(ws * S), / S, * 2 - 1 with S = 2^bits - 1, every step one f32
                                 rounding, torch.round = half to even (oracle/encoder.py quantize_uniform /
                                 uniform_indices)
  argmin(z, cb)    -> idx        torch.argmin(|z - c|) on f32 distances: the first index on ties, 0 for a NaN or
                                 infinite latent (every distance is then NaN or inf: all equal, or NaN first)
  lookup(codes, cb) -> (w, oob)  cb[code]; a code outside [0, k) gives 0 and sets the flag

Soft values get an fp64 reference from the f32 operands, and a bound per element: gumbel().

The bound of gumbel(), counted on the kernel's f32 roundings (u = 2^-24, every rounding relative u; expf within one
ulp = 2u).  Per row, with d_k = |z - c_k|, y_k = (-d_k + g_k) / tau, Y = max_k |y_k|, D = max_k d_k / tau and
W = max(Y, D):

  y       the subtraction (u d_k / tau), the add of g (u |y_k|), inv_tau = 1 / tau (u |y_k|; tau = expf(log_tau)
          adds 2u |y_k| where the temperature is given as its logarithm) and the product with it (u |y_k|):
              |dy_k| <= u (D + 5 Y)
  p       a_k = y_k - ymax is one rounding of a value of at most 2Y (2u Y), expf 2u, the k-term sum of positive
          terms (KPL - 1 <= 15 adds in the lane, 6 levels across the wave: 21u), 1 / s (u) and e * inv_s (u).  The
          error of ymax is common to the numerator and the denominator and cancels; what remains is counted once in
          each:
              |dp_k| / p_k <= 2 (u (D + 5 Y) + 2u Y) + (2 + 1 + 1) u + (2 + 21) u = u (27 + 14 Y + 2 D)
  disc    the product with c_k (u) and the sum (15 + 6 adds: 21u) of terms whose magnitudes add up to at most max|c|:
              |disc - ref| <= u (49 + 14 Y + 2 D) max|c|  <=  K_disc u (1 + W) max|c|,    K_disc = 49
  psum    per column, the rows' p_k (each to the relative error above, taken at the largest Y and D of the call), then
          a chain of f32 additions of positive terms onto the caller's prefill: the trips of one wave's grid-stride
          loop, the 3 adds over a workgroup's 4 waves and one float atomic per workgroup, in any order:
              |psum_k - (pre_k + ref_k)| <= u (K_psum (1 + W_max) + terms) (|pre_k| + ref_k) + n 2^-126,
              K_psum = 27,  terms = trips + 3 + workgroups
          (2^-126 per row: below the smallest normal f32, expf has no relative precision left; the fp64 reference
          keeps such a probability, the kernel may hold 0.)

The shape is the one of "K u (1 + Y) max|c|" with W in the place of Y: d_k / tau is not bounded by Y when the noise
cancels the distance, so the first rounding is measured by D.  Every term comes from the fp64 reference.

Hard mode: ret = ((1 - p) + p) at the chosen entry is exactly 1 in f32 (1 - p is within 2^-25 of its value, the sum
within 2^-25 of 1, and rounds to 1), and ((0 - p) + p) is exactly 0 elsewhere, so disc = c[argmax y].  The argmax is a
decision on rounded y: a row is unambiguous when the fp64 gap between the two largest y exceeds the error of their
difference, u (2 D + 4 Y) (the subtraction twice, the add and the product twice each; 1 / tau is common and does not
reorder).  The tests use 16 u Y, or this where it is larger.
"""
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
K_DISC_DERIVED = 49.0
K_PSUM_DERIVED = 27.0
GUMBEL_GRID_CAP = 4096      # workgroups of 4 waves, one latent per wave and trip
ARGMIN_CHUNK = 1 << 26      # elements of the [rows, k] distance matrix held at once


def uniform(w, bits):
    """(q f32, idx int64) of the uniform n-bit quantizer, f32 op order as written in the reference."""
    assert w.dtype == torch.float32
    s = float((1 << bits) - 1)
    ws = (w + 1.0) * 0.5
    r = torch.round(ws * s)
    q = (r / s) * 2.0 - 1.0
    return q, r.to(torch.int64)


def argmin(z, cb):
    """idx int64 [z.numel()]: torch.argmin of the f32 distances, chunked over z."""
    assert z.dtype == torch.float32 and cb.dtype == torch.float32
    z = z.reshape(-1)
    k = cb.numel()
    rows = max(1, ARGMIN_CHUNK // k)
    out = torch.empty(z.numel(), dtype=torch.int64)
    for lo in range(0, z.numel(), rows):
        d = torch.abs(z[lo:lo + rows].reshape(-1, 1) - cb.reshape(1, -1))
        out[lo:lo + rows] = torch.argmin(d, dim=1)
    return out


def lookup(codes, cb):
    """(w f32, oob bool): cb[code], 0 and the flag for codes outside [0, k)."""
    codes = codes.reshape(-1)
    k = cb.numel()
    bad = (codes < 0) | (codes >= k)
    w = cb[torch.where(bad, torch.zeros_like(codes), codes)]
    w = torch.where(bad, torch.zeros_like(w), w)
    return w, bool(bad.any())


def gumbel_terms(n, grid_cap=GUMBEL_GRID_CAP):
    """Additions in the chain that forms one column sum: trips of a wave, 3 across the waves, one per workgroup."""
    groups = min(-(-n // 4), grid_cap)
    trips = -(-n // (4 * groups))
    return trips + 3 + groups


def gumbel_rows(z, cb, noise, tau):
    """The per-row part of gumbel(), shared by both modes and by every prefix of the rows."""
    assert z.dtype == torch.float32 and cb.dtype == torch.float32 and noise.dtype == torch.float32
    z = z.reshape(-1)
    n, k = z.numel(), cb.numel()
    c = cb.double()
    d = torch.abs(z.double().reshape(-1, 1) - c.reshape(1, -1))
    y = (-d + noise.double().reshape(n, k)) / tau
    p = torch.softmax(y, dim=1)
    top1 = torch.argmax(y, dim=1)           # first index on ties, as torch.max and the kernel
    if k > 1:
        ym = y.clone()
        ym[torch.arange(n), top1] = -float("inf")
        top2 = torch.argmax(ym, dim=1)
        gap = y[torch.arange(n), top1] - y[torch.arange(n), top2]
    else:
        top2 = top1.clone()
        gap = torch.full([n], float("inf"), dtype=torch.float64)
    Y = y.abs().amax(dim=1)
    D = d.amax(dim=1) / tau
    return dict(idx=argmin(z, cb), p=p, c=c, disc_soft=(p * c.reshape(1, -1)).sum(1), top1=top1, top2=top2, gap=gap,
                Y=Y, D=D, W=torch.maximum(Y, D), ambiguous=gap <= U * torch.maximum(16.0 * Y, 2.0 * D + 4.0 * Y))


def gumbel(z, cb, noise, tau, hard, rows=None, n=None):
    """fp64 reference of the Gumbel-softmax quantizer forward from f32 operands (tau: a Python float, the value the
    kernel is given, or exp of the f32 logarithm in fp64) -> dict of
      idx        the f32 argmin oracle                                   [n] int64
      disc       sum_k p_k c_k (soft), c[top1] (hard)                    [n] f64
      top1, top2 indices of the two largest y (first index on ties), gap their fp64 difference (inf when k = 1)
      Y, D, W    per row, as in the module docstring
      psum       column sums of p (soft) or of the one-hot at top1 (hard) [k] f64
      ambiguous  gap <= u max(16 Y, 2 D + 4 Y)
      disc_bound(K), psum_bound(K, pre): the bounds of the module docstring.
    rows: a gumbel_rows() result to reuse; n: only its first n rows (the kernel's rows are independent)."""
    r = gumbel_rows(z, cb, noise, tau) if rows is None else rows
    n = r["Y"].numel() if n is None else n
    k = r["c"].numel()
    c = r["c"]
    cmax = c.abs().max().item()
    out = {key: r[key][:n] for key in ("idx", "top1", "top2", "gap", "Y", "D", "W", "ambiguous", "p")}
    W = out["W"]
    if hard:
        disc = c[out["top1"]]
        nan_rows = out["p"].isnan().any(dim=1)
        disc = torch.where(nan_rows, torch.full_like(disc, float("nan")), disc)
        psum = torch.bincount(out["top1"], minlength=k).double()
        if bool(nan_rows.any()):
            psum = torch.full_like(psum, float("nan"))
    else:
        disc = r["disc_soft"][:n]
        psum = out["p"].sum(0)
    w_max = W.max().item()
    terms = gumbel_terms(n)

    def disc_bound(K):
        return K * U * (1.0 + W) * cmax + k * TINY * cmax

    def psum_bound(K, pre=None):
        base = psum if pre is None else psum + pre.double().abs()
        return U * (K * (1.0 + w_max) + terms) * base + n * TINY

    out.update(c=c, disc=disc, psum=psum, disc_bound=disc_bound, psum_bound=psum_bound, terms=terms, cmax=cmax,
               w_max=w_max)
    return out


# ------------------------------------------------------------------------------------------ input builders (CPU)
def uniform_grid(bits, count=None, seed=0):
    """(w, r): the exact grid points (r / S) * 2 - 1 in f32 for every r in 0..S, or `count` random ones."""
    s = (1 << bits) - 1
    if count is None or count > s:
        r = torch.arange(s + 1, dtype=torch.int64)
    else:
        r = torch.randint(0, s + 1, [count], generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    w = (r.float() / float(s)) * 2.0 - 1.0
    return w, r


def uniform_halfway(bits, count=4096, seed=0):
    """(w, r): f32 w whose f32 product ((w + 1) * 0.5) * S is exactly r + 0.5, found by searching the f32 neighbours
    of (2 (r + 0.5) / S) - 1; only exact hits are kept.  r even and odd both occur (asserted by the caller)."""
    s = (1 << bits) - 1
    if s <= count:
        r = torch.arange(s, dtype=torch.int64)
    else:
        r = torch.randint(0, s, [count], generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
        r = torch.cat([r, torch.tensor([0, 1, s - 2, s - 1])])
    if bits == 24:
        # r + 0.5 is not an f32 above 2^23: only the lower half of the range has half-way points
        r = r[r < (1 << 23)]
    target = r.double() + 0.5
    w0 = (2.0 * target / s - 1.0).float()
    found_w, found_r = [], []
    cand = w0.clone()
    for _ in range(4):
        cand = torch.nextafter(cand, torch.full_like(cand, -2.0))
    for _ in range(9):
        prod = ((cand + 1.0) * 0.5) * float(s)
        hit = prod.double() == target
        found_w.append(cand[hit])
        found_r.append(r[hit])
        cand = torch.nextafter(cand, torch.full_like(cand, 2.0))
    w = torch.cat(found_w)
    rr = torch.cat(found_r)
    return w, rr


def midpoints(cb):
    """(c_j + c_{j+1}) / 2 in f32 for the sorted entries (k - 1 values; empty for k = 1)."""
    s = torch.sort(cb).values
    return (s[:-1] + s[1:]) / 2.0


def codebook_shuffled(k, seed=0):
    """linspace(-1, 1, k) shuffled, then three entries overwritten with copies of three others (k >= 6), so that each
    duplicated value occurs at two indices and the first must win."""
    g = torch.Generator().manual_seed(seed)
    cb = torch.linspace(-1, 1, k).float()[torch.randperm(k, generator=g)]
    if k >= 6:
        pos = torch.randperm(k, generator=g)[:6]
        cb[pos[3:]] = cb[pos[:3]]
    return cb.contiguous()
