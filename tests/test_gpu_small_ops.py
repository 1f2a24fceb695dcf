"""Kernel-level tests of the small ops that only whole-encoder / whole-generator runs reached: each C ABI entry
point is called directly (ctypes) and compared with a plain float64 CPU reference of the same operation, computed from
the operands after they are rounded to the kernel's input type.

Every output buffer is a slice of a larger allocation: the slice has exactly the size the entry point's `*_floats`
query (or its documented output shape) gives, it is prefilled with NaN, and the guard elements on both sides hold a
sentinel bit pattern that must survive the call.  All of that is memory this file allocated."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guarded import Guarded, _bits, _nan_bits, _same_bits
from image_compression_2_amd import _native as nv
from oracle import sg3

pytestmark = pytest.mark.gpu

U = 2.0 ** -24      # unit roundoff of f32 (half an ulp of a value in [1, 2))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ====================================================================================== 1. ic2_reparameterize
# grid_1d of encoder_ops.hip caps the launch at 8192 workgroups of 256 threads: the last shape is the smallest n for
# which n * 7 * 512 elements need more (585 * 3584 = 2,096,640 <= 8192 * 256 = 2,097,152 < 586 * 3584 = 2,100,224), so
# the grid-stride loop runs a second time for the tail.  (It also passes the 4096 * 256 of a 4096-block cap.)
REPARAM_GRID_CAP = 8192
REPARAM_SHAPES = [(2, 3, 5, 3, 0), (3, 5, 512, 16, 5), (1, 4, 33, 16, 12), (586, 7, 512, 16, 5)]
# logvar columns d % 11 == 0 .. 4 hold these values (the other columns are random): expf(0.5 * lv) is tiny at -120,
# underflows to 0 at -250, is 1 at 0, 4.9e8 at +40 and overflows to inf at +200
REPARAM_LV = [-120.0, 0.0, 40.0, 200.0, -250.0]
# |w - fp64| <= K * 2^-24 * (|m| + |eps * sd|): the product eps * expf(0.5 lv) and the sum are one f32 rounding each,
# expf adds its own error.  Measured on MI355X over these inputs: max ratio 2.70 (the 586 x 7 x 512 case); 2x margin.
REPARAM_K = 5.4


def _reparam_inputs(n, num_ws, w_dim, seed):
    g = _gen(seed)
    params = torch.randn(n, num_ws, 2 * w_dim, generator=g)
    params[..., w_dim:] *= 2.0
    d = torch.arange(w_dim)
    for j, lv in enumerate(REPARAM_LV):
        cols = (d % 11 == j).nonzero().flatten() + w_dim
        params[..., cols] = lv
    eps = torch.randn(n, num_ws, w_dim, generator=g)
    # |eps| >= 1e-3: at lv = +200 the kernel's eps * inf is +-inf for every non-zero eps, while the fp64 product
    # eps * e^100 only passes the f32 range for |eps| > 1.3e-5; keep the two on the same side
    eps = torch.where(eps.abs() < 1e-3, torch.full_like(eps, 1e-3), eps)
    return params, eps


def _reparam_call(cuda, params, eps, n, num_ws, w_dim, ws_total, ws_off, want=(True, True, True)):
    outs = [Guarded(n * ws_total * w_dim, torch.float32, cuda) if k else None for k in want]
    pd = params.to(cuda)
    ed = None if eps is None else eps.to(cuda)
    nv.call("ic2_reparameterize", nv.ptr(pd), nv.ptr(ed), n, num_ws, w_dim, ws_total, ws_off,
            *[None if o is None else o.ptr() for o in outs], nv.stream_of(pd))
    torch.cuda.synchronize()
    for o in outs:
        assert o is None or o.intact()
    return [None if o is None else o.t.view(n, ws_total, w_dim).cpu() for o in outs]


@pytest.mark.parametrize("n,num_ws,w_dim,ws_total,ws_off", REPARAM_SHAPES)
def test_reparameterize(cuda, n, num_ws, w_dim, ws_total, ws_off):
    total = n * num_ws * w_dim
    if n == REPARAM_SHAPES[-1][0]:   # the grid-stride case: just past the cap, and the smallest such n
        assert (n - 1) * num_ws * w_dim <= REPARAM_GRID_CAP * 256 < total
    # a ragged last workgroup where w_dim is 5 or 33 (512-wide rows always fill whole workgroups of 256)
    assert [a * b * c % 256 != 0 for a, b, c, _, _ in REPARAM_SHAPES] == [True, False, True, False]
    params, eps = _reparam_inputs(n, num_ws, w_dim, seed=w_dim + n)
    assert bool((eps != 0).all())
    w, mean, logvar = _reparam_call(cuda, params, eps, n, num_ws, w_dim, ws_total, ws_off)
    rows = slice(ws_off, ws_off + num_ws)
    outside = torch.ones(ws_total, dtype=torch.bool)
    outside[rows] = False
    for out in (w, mean, logvar):    # rows of other projectors keep the prefill
        assert bool(_nan_bits(out[:, outside]).all())
    assert _same_bits(mean[:, rows], params[..., :w_dim])
    assert _same_bits(logvar[:, rows], params[..., w_dim:])
    m, lv, e = params[..., :w_dim].double(), params[..., w_dim:].double(), eps.double()
    ref = m + e * torch.exp(0.5 * lv)
    ref32 = ref.float()
    got = w[:, rows]
    assert not bool(got.isnan().any())
    inf = ref32.isinf()
    d = torch.arange(w_dim)
    assert bool(inf[..., d % 11 == 3].all()) and not bool(inf[..., d % 11 != 3].any())   # overflow exactly at +200
    assert torch.equal(got[inf], ref32[inf])            # the same +-inf
    assert bool(got[~inf].isfinite().all())
    fin = ~inf
    bound = U * (m.abs() + (e * torch.exp(0.5 * lv)).abs())
    ratio = ((got.double() - ref).abs()[fin] / bound[fin]).max().item()
    print(f"[reparameterize {n}x{num_ws}x{w_dim}] max |w - fp64| / (2^-24 (|m| + |eps sd|)) = {ratio:.3f}")
    assert ratio <= REPARAM_K
    # sd underflows to 0 at lv = -250: w is the mean itself
    assert _same_bits(got[..., d % 11 == 4], params[..., :w_dim][..., d % 11 == 4])
    # eps == NULL: w is the mean, bit for bit
    w0, _, _ = _reparam_call(cuda, params, None, n, num_ws, w_dim, ws_total, ws_off, want=(True, False, False))
    assert _same_bits(w0[:, rows], params[..., :w_dim])


@pytest.mark.parametrize("want", [(False, True, True), (True, False, True), (True, True, False),
                                  (False, False, True), (False, False, False)])
def test_reparameterize_null_outputs(cuda, want):
    """Each output may be NULL independently; the ones that are given do not change."""
    n, num_ws, w_dim, ws_total, ws_off = REPARAM_SHAPES[2]
    params, eps = _reparam_inputs(n, num_ws, w_dim, seed=5)
    full = _reparam_call(cuda, params, eps, n, num_ws, w_dim, ws_total, ws_off)
    part = _reparam_call(cuda, params, eps, n, num_ws, w_dim, ws_total, ws_off, want=want)
    for k, a, b in zip(want, part, full):
        assert (a is None) == (not k)
        assert a is None or _same_bits(a, b)


# ====================================================================== 2. ic2_global_avg_pool, f32 / bf16 / f16
GAP_CHUNK = 64   # pixels per partial sum (encoder_ops.hip)
GAP_SHAPES = [(2, 1, 20, 32), (3, 63, 32, 32), (1, 64, 96, 96), (2, 65, 270, 288), (2, 1091, 40, 64)]


def test_gap_shapes_reach_every_path():
    """What the shapes are there for, stated on the shapes alone."""
    chunks = [math.ceil(hw / GAP_CHUNK) for _, hw, _, _ in GAP_SHAPES]
    assert max(chunks) > 16                                    # the finalize kernel's 16 chunk lanes wrap
    assert 1 in chunks and 2 in chunks                         # one full chunk / one pixel past it
    assert any(hw == GAP_CHUNK for _, hw, _, _ in GAP_SHAPES)
    assert any(c_p > 256 for *_, c_p in GAP_SHAPES)            # a second blockIdx.x of the partial kernel
    assert sum(c % 16 != 0 for _, _, c, _ in GAP_SHAPES) >= 2  # ragged 16-channel finalize blocks
    assert any(c < c_p for _, _, c, c_p in GAP_SHAPES)


def _gap_input(n, hw, c, c_p, dtype, seed):
    x = torch.full([n, hw, c_p], 1e4)       # padded channels: large finite garbage that must not leak
    x[..., :c] = torch.randn(n, hw, c, generator=_gen(seed)) * 2 + 0.7
    return x.to(dtype)


@pytest.mark.parametrize("n,hw,c,c_p", GAP_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_global_avg_pool(cuda, n, hw, c, c_p, dtype):
    x = _gap_input(n, hw, c, c_p, dtype, seed=hw + c)
    nchunks = math.ceil(hw / GAP_CHUNK)
    nfl = int(nv.query("ic2_global_avg_pool_floats", n, hw, c_p, c))
    assert nfl == n * c + n * nchunks * c_p
    out = Guarded(nfl, torch.float32, cuda)
    xd = x.to(cuda)
    nv.call("ic2_global_avg_pool", nv.ptr(xd), nv.dtype_code(dtype), n, hw, c_p, c, out.ptr(), nv.stream_of(xd))
    torch.cuda.synchronize()
    assert out.intact()
    got = out.t[:n * c].view(n, c).cpu()
    assert bool(got.isfinite().all())
    xr = x.double()[..., :c]
    ref = xr.mean(dim=1)
    # summation structure: <= 64 sequential f32 adds per chunk, ceil(nchunks / 16) adds per chunk lane, a 16-term
    # lane sum and the division, each at most 2^-24 of the sum of magnitudes
    bound = (GAP_CHUNK + math.ceil(nchunks / 16) + 16 + 1) * U * xr.abs().mean(dim=1)
    err = (got.double() - ref).abs()
    print(f"[gap {dtype} n{n} hw{hw} c{c}] max err / bound = {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    assert float(ref.abs().mean()) > 100 * float(bound.max())   # a dropped pixel or chunk is far outside


# ============================================================================ 3. ic2_gap_bwd, f32 / bf16 / f16
GAPB_REL = {torch.float32: 2.0 ** -22,                  # 1 / hw rounded, then one multiply
            torch.bfloat16: 2.0 ** -22 + 2.0 ** -8,     # plus one rounding of the out type
            torch.float16: 2.0 ** -22 + 2.0 ** -11}


def _gap_bwd(cuda, dp, n, hw, c, c_p, dtype):
    dx = Guarded(n * hw * c_p, dtype, cuda)
    dpd = dp.to(cuda)
    nv.call("ic2_gap_bwd", nv.ptr(dpd), dx.ptr(), nv.dtype_code(dtype), n, hw, c_p, c, nv.stream_of(dpd))
    torch.cuda.synchronize()
    assert dx.intact()
    return dx.t.view(n, hw, c_p).cpu()


@pytest.mark.parametrize("n,hw,c,c_p", GAP_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gap_bwd(cuda, n, hw, c, c_p, dtype):
    g = _gen(hw * 3 + c)
    # 0.25 <= |dp| < 1.25: dp / hw stays in f16's normal range (>= 2.3e-4 at hw = 1091), so the relative bound holds
    dp = (torch.rand(n, c, generator=g) + 0.25) * (torch.randint(0, 2, [n, c], generator=g) * 2 - 1).float()
    got = _gap_bwd(cuda, dp, n, hw, c, c_p, dtype)
    assert bool(got[..., :c].isfinite().all())
    ref = (dp.double() / hw)[:, None, :].expand(n, hw, c)
    rel = ((got[..., :c].double() - ref).abs() / ref.abs()).max().item()
    print(f"[gap_bwd {dtype} n{n} hw{hw} c{c}] max relative error {rel:.3e} (bound {GAPB_REL[dtype]:.3e})")
    assert rel <= GAPB_REL[dtype]
    assert bool((_bits(got[..., c:]) == 0).all())          # padded channels: +0, bit for bit
    # a loss-scaled gradient past the f16 range reaches the scaler as inf (IEEE conversion, no saturation)
    big = _gap_bwd(cuda, torch.full([n, c], 7e4 * hw), n, hw, c, c_p, dtype)
    if dtype == torch.float16:
        assert bool((big[..., :c] == float("inf")).all())
    else:
        assert bool(big[..., :c].isfinite().all())
        assert float((big[..., :c].double() / 7e4 - 1).abs().max()) <= GAPB_REL[dtype]
    assert bool((_bits(big[..., c:]) == 0).all())


# ============================================================================================ 4. layout converters
LAYOUT_SHAPES = [(2, 3, 5, 7, 32), (1, 40, 9, 4, 64), (3, 33, 1, 11, 64)]   # h != w throughout


def _to_nhwc(cuda, x, code, n, c, h, w, c_p, scale, elem_dtype, per_pixel):
    y = Guarded(n * h * w * per_pixel, elem_dtype, cuda)
    xd = x.to(cuda)
    sd = None if scale is None else scale.to(cuda)
    nv.call("ic2_nchw_to_nhwc", nv.ptr(xd), y.ptr(), code, n, c, h, w, c_p, nv.ptr(sd), nv.stream_of(xd))
    torch.cuda.synchronize()
    assert y.intact()
    return y.t.view(n, h, w, per_pixel).cpu()


@pytest.mark.parametrize("n,c,h,w,c_p", LAYOUT_SHAPES)
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("dtype", DTYPES + ["split"])
def test_nchw_to_nhwc(cuda, n, c, h, w, c_p, scaled, dtype):
    assert h != w
    g = _gen(c * 11 + h)
    x = torch.randn(n, c, h, w, generator=g)
    scale = torch.randn(n, c_p, generator=g) if scaled else None
    v = F.pad(x.permute(0, 2, 3, 1), (0, c_p - c))             # NHWC f32, zero padded
    if scaled:
        v = v * scale[:, None, None, :]                        # the product in f32, before any rounding
    if dtype == "split":
        got = _to_nhwc(cuda, x, nv.BF16X3, n, c, h, w, c_p, scale, torch.bfloat16, 2 * c_p)
        hi = v.to(torch.bfloat16)
        lo = (v - hi.float()).to(torch.bfloat16)
        assert _same_bits(got[..., :c_p], hi)
        assert _same_bits(got[..., c_p:], lo)
    else:
        got = _to_nhwc(cuda, x, nv.dtype_code(dtype), n, c, h, w, c_p, scale, dtype, c_p)
        assert _same_bits(got, v.to(dtype))                    # round to nearest even, padding included
    if not scaled:
        assert bool((_bits(got.contiguous()).view(n, h, w, -1, c_p)[..., c:] == 0).all())   # +0 padding


@pytest.mark.parametrize("n,c,h,w,c_p", LAYOUT_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nhwc_to_nchw(cuda, n, c, h, w, c_p, dtype):
    assert h != w
    x = torch.full([n, h, w, c_p], 1e4)                        # padded channels: garbage that must not be read out
    x[..., :c] = torch.randn(n, h, w, c, generator=_gen(c + w))
    x = x.to(dtype)
    y = Guarded(n * c * h * w, torch.float32, cuda)
    xd = x.to(cuda)
    nv.call("ic2_nhwc_to_nchw", nv.ptr(xd), nv.dtype_code(dtype), y.ptr(), n, c, h, w, c_p, nv.stream_of(xd))
    torch.cuda.synchronize()
    assert y.intact()
    assert _same_bits(y.t.view(n, c, h, w).cpu(), x[..., :c].float().permute(0, 3, 1, 2).contiguous())


@pytest.mark.parametrize("n,c,h,w,c_p", LAYOUT_SHAPES)
def test_layout_round_trip_is_identity(cuda, n, c, h, w, c_p):
    x = torch.randn(n, c, h, w, generator=_gen(w))
    mid = _to_nhwc(cuda, x, nv.F32, n, c, h, w, c_p, None, torch.float32, c_p)
    back = Guarded(n * c * h * w, torch.float32, cuda)
    md = mid.to(cuda)
    nv.call("ic2_nhwc_to_nchw", nv.ptr(md), nv.F32, back.ptr(), n, c, h, w, c_p, nv.stream_of(md))
    torch.cuda.synchronize()
    assert back.intact()
    assert _same_bits(back.t.view(n, c, h, w).cpu(), x)


# ======================================================================================= 5. ic2_synth_input_features
SYNTH_SR, SYNTH_BW = 16.0, 2.0
SYNTH_CASES = [(3, 20, 32, 10), (2, 300, 320, 7), (1, 64, 64, 36)]
# Two bounds on |out - fp64|, both asserted.
# (a) C1 * 2^-23 * (1 + |2 pi arg|) * amp.  The argument is a sum of three terms (x f0' + y f1' + phase') of up to
#     ~60 rad each that may cancel, and its f32 error follows the terms, not the sum: measured on MI355X over these
#     inputs the ratio is at most 47.6 (size 36, 2x transform, at a near-zero argument); 2x margin.
# (b) C2 * 2^-23 * ((1 + mag) * amp + amp_err): `mag` is the same argument with every product and sum taken in
#     magnitudes (what the f32 rounding errors are relative to), amp_err = 1 + |f'| / (sr / 2 - bw) where the amplitude
#     is strictly between its clamps (its f32 error is absolute, a few 2^-24 of the terms of 1 - (|f'| - bw) / (..)),
#     0 where it is clamped.  Measured max ratio 1.73 (0.96 .. 1.73 over the six f32 cases); 2x margin.
SYNTH_C1 = 96.0
SYNTH_C2 = 3.5


def _synth_ref(t, freqs, phases, tr, size, sr, bw):
    """SynthesisInput.forward after the affine layer, in the operands' dtype (float64 here):
    -> (features [n, size, size, c] NHWC, 2 pi * argument of the sine, amplitudes [n, c], the argument's magnitude
    sum [n, size, size, c], |rotated frequency| [n, c])."""
    n = t.shape[0]
    t = t / t[:, :2].norm(dim=1, keepdim=True)
    m_r = torch.eye(3, dtype=t.dtype).repeat(n, 1, 1)       # rotation by the normalised (t0, t1)
    m_r[:, 0, 0], m_r[:, 0, 1], m_r[:, 1, 0], m_r[:, 1, 1] = t[:, 0], -t[:, 1], t[:, 1], t[:, 0]
    m_t = torch.eye(3, dtype=t.dtype).repeat(n, 1, 1)       # inverse translation
    m_t[:, 0, 2], m_t[:, 1, 2] = -t[:, 2], -t[:, 3]
    m = m_r @ m_t @ tr[None]
    ph = phases[None] + (freqs[None] @ m[:, :2, 2:]).squeeze(2)
    fr = freqs[None] @ m[:, :2, :2]                          # [n, c, 2]
    amp = (1 - (fr.norm(dim=2) - bw) / (sr / 2 - bw)).clamp(0, 1)
    # affine_grid(align_corners=False) scaled by theta = 0.5 size / sr: pixel centres, x along the width
    gxy = ((2 * torch.arange(size, dtype=t.dtype) + 1) / size - 1) * (0.5 * size / sr)
    arg = (gxy[None, None, :, None] * fr[:, None, None, :, 0] + gxy[None, :, None, None] * fr[:, None, None, :, 1]
           + ph[:, None, None, :]) * (2 * math.pi)
    fa = freqs.abs()[None] @ m[:, :2, :2].abs()
    pa = phases.abs()[None] + (freqs.abs()[None] @ m[:, :2, 2:].abs()).squeeze(2)
    mag = (gxy.abs()[None, None, :, None] * fa[:, None, None, :, 0] + gxy.abs()[None, :, None, None]
           * fa[:, None, None, :, 1] + pa[:, None, None, :]) * (2 * math.pi)
    return torch.sin(arg) * amp[:, None, None, :], arg, amp, mag, fr.norm(dim=2)


def _synth_operands(n, c, seed):
    g = _gen(seed)
    # frequencies of radius 0 .. 5 = 2.5 x the bandwidth, kept 0.03 clear of the radii (1, 2, 4) at which the amplitude
    # clamp switches for a 1x / 2x user transform, so f32 and f64 stand on the same side of every switch
    r = torch.rand(c, generator=g, dtype=torch.float64) * 5
    for edge in (1.0, 2.0, 4.0):
        r = torch.where((r - edge).abs() < 0.03, torch.full_like(r, edge + 0.05), r)
    a = torch.rand(c, generator=g, dtype=torch.float64) * (2 * math.pi)
    freqs = torch.stack([r * torch.cos(a), r * torch.sin(a)], dim=1).float()
    phases = (torch.rand(c, generator=g) - 0.5)
    # t = 1.7 (cos 37, sin 37) (not normalised: the kernel divides), translation (0.3, -0.2), varied per sample
    t = torch.empty(n, 4)
    for i in range(n):
        ang = math.radians(37.0 + 61.0 * i)
        t[i] = torch.tensor([1.7 * math.cos(ang), 1.7 * math.sin(ang), 0.3 + 0.11 * i, -0.2 - 0.07 * i])
    return t, freqs, phases


def _user_transform(kind):
    if kind == "identity":
        return torch.eye(3)
    ang = math.radians(23.0)                                 # rotation + translation + 2x scale
    return torch.tensor([[2 * math.cos(ang), -2 * math.sin(ang), 0.15], [2 * math.sin(ang), 2 * math.cos(ang), -0.4],
                         [0.0, 0.0, 1.0]])


def test_synth_input_restatement_agrees_with_oracle():
    """_synth_ref against oracle/sg3.synthesis_input with an identity affine layer and an identity channel mix."""
    n, c, _, size = SYNTH_CASES[0]
    t, freqs, phases = _synth_operands(n, c, seed=c)
    tr = _user_transform("scaled")
    sd = {"synthesis.input.freqs": freqs, "synthesis.input.phases": phases, "synthesis.input.transform": tr,
          "synthesis.input.affine.weight": torch.eye(4) * 2.0,      # fully_connected scales by 1 / sqrt(4)
          "synthesis.input.affine.bias": torch.zeros(4),
          # ... and the channel mix by 1 / sqrt(c)
          "synthesis.input.weight": torch.eye(c, dtype=torch.float64) * math.sqrt(c)}
    inp = {"sampling_rate": SYNTH_SR, "bandwidth": SYNTH_BW, "size": size, "channels": c}
    ora = sg3.synthesis_input(sd, inp, t.double(), dtype=torch.float64)          # NCHW
    mine, *_ = _synth_ref(t.double(), freqs.double(), phases.double(), tr.double(), size, SYNTH_SR, SYNTH_BW)
    assert ora.shape == (n, c, size, size)
    assert float((ora.permute(0, 2, 3, 1) - mine).abs().max()) < 1e-12


@pytest.mark.parametrize("n,c,c_p,size", SYNTH_CASES)
@pytest.mark.parametrize("user", ["identity", "scaled"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_synth_input_features(cuda, n, c, c_p, size, user, dtype):
    t, freqs, phases = _synth_operands(n, c, seed=c)
    tr = _user_transform(user)
    ref, arg, amp, mag, fnorm = _synth_ref(t.double(), freqs.double(), phases.double(), tr.double(), size, SYNTH_SR,
                                           SYNTH_BW)
    # the clamp is exercised on both sides (the scaled transform pushes channels past the cutoff)
    assert bool((amp == 1).any()) and bool(((amp > 0) & (amp < 1)).any())
    if user == "scaled":
        assert bool((amp == 0).any())
    out = Guarded(n * size * size * c_p, dtype, cuda)
    dev = [v.to(cuda) for v in (t, freqs, phases, tr)]
    nv.call("ic2_synth_input_features", *[nv.ptr(v) for v in dev], n, c, c_p, size, SYNTH_SR, SYNTH_BW, out.ptr(),
            nv.dtype_code(dtype), nv.stream_of(dev[0]))
    torch.cuda.synchronize()
    assert out.intact()
    got = out.t.view(n, size, size, c_p).cpu()
    assert bool(got.isfinite().all())
    assert bool((_bits(got[..., c:]) == 0).all())              # padded channels: +0
    err = (got[..., :c].double() - ref).abs()
    amp4 = amp[:, None, None, :]
    amp_err = torch.where((amp > 0) & (amp < 1), 1 + fnorm / (SYNTH_SR / 2 - SYNTH_BW), torch.zeros_like(amp))
    bound_a = 2.0 ** -23 * (1 + arg.abs()) * amp4
    bound_b = 2.0 ** -23 * ((1 + mag) * amp4 + amp_err[:, None, None, :])
    if dtype == torch.float32:
        pos = amp4.expand_as(err) > 0
        print(f"[synth_input n{n} c{c} s{size} {user}] max err / (2^-23 (1 + |2 pi arg|) amp) = "
              f"{(err[pos] / bound_a[pos]).max().item():.3f}, max err / bound (b) = "
              f"{(err[pos] / bound_b[pos]).max().item():.3f}")
        half_ulp = torch.zeros_like(ref)
    elif dtype == torch.bfloat16:
        half_ulp = 2.0 ** -8 * ref.abs()                                 # 8-bit significand
    else:
        half_ulp = torch.clamp(2.0 ** -11 * ref.abs(), min=2.0 ** -25)   # 11 bits; subnormal spacing 2^-24
    assert bool((err <= SYNTH_C1 * bound_a + half_ulp).all())
    assert bool((err <= SYNTH_C2 * bound_b + half_ulp).all())


# ============================================================================== 6. ic2_modconv_prep against the formula
MODCONV_CASES = [(1, 3, 32, 5, 32), (5, 362, 384, 256, 256), (3, 1024, 1024, 130, 160), (2, 512, 512, 3, 32)]


@pytest.mark.parametrize("n,cin,cin_p,cout,cout_p", MODCONV_CASES)
@pytest.mark.parametrize("demod", [0, 1])
def test_modconv_prep_matches_formula(cuda, n, cin, cin_p, cout, cout_p, demod):
    g = _gen(cin + cout)
    s = torch.randn(n, cin, generator=g) * 1.5 + 0.2
    wsq = torch.rand(cout, cin, generator=g) + 0.1
    style_gain, input_gain = 0.37, 1.3
    xs = Guarded(n * cin_p, torch.float32, cuda)
    os_ = Guarded(n * cout_p, torch.float32, cuda)
    sd, wd = s.to(cuda), wsq.to(cuda)
    nv.call("ic2_modconv_prep", nv.ptr(sd), nv.ptr(wd), n, cin, cout, cin_p, cout_p, demod, style_gain, input_gain,
            xs.ptr(), os_.ptr(), None, nv.stream_of(sd))
    torch.cuda.synchronize()
    assert xs.intact() and os_.intact()
    gx, go = xs.t.view(n, cin_p).cpu(), os_.t.view(n, cout_p).cpu()
    assert bool(gx.isfinite().all()) and bool(go.isfinite().all())
    assert bool((gx[:, cin:] == 0).all()) and bool((go[:, cout:] == 0).all())
    s64 = s.double()
    gain = s64.square().mean().rsqrt() if demod else torch.tensor(float(np.float32(style_gain)), dtype=torch.float64)
    xref = s64 * gain
    ig = float(np.float32(input_gain))
    if demod:
        oref = ig * (xref.square() @ wsq.double().t() + 1e-8).rsqrt()
    else:
        oref = torch.full([n, cout], ig, dtype=torch.float64)
    xrel = ((gx[:, :cin].double() - xref).abs() / xref.abs()).max().item()
    orel = ((go[:, :cout].double() - oref).abs() / oref.abs()).max().item()
    # xscale: the f32 rounding of the mean (halved by the rsqrt), rsqrtf (<= 1 ulp) and the product.  oscale: 64 lanes
    # each sum ceil(cin / 64) positive terms in f32, a 6-step tree, + 1e-8, rsqrtf, the gain; the terms carry xscale's
    # error twice and two product roundings (halved by the rsqrt)
    xtol, otol = 4 * U, (math.ceil(cin / 64) + 6 + 4) * U
    print(f"[modconv_prep n{n} cin{cin} cout{cout} demod{demod}] xscale rel {xrel / U:.2f} u (<= 4), "
          f"oscale rel {orel / U:.2f} u (<= {otol / U:.0f})")
    assert xrel <= xtol
    assert orel <= otol


# ==================================================================== 7. ic2_conv_wgrad / ic2_conv_wgrad_oihw, direct
# The last case makes both kernels split the pixel axis unevenly.  P = 2 * 32 * 41 = 2624 output pixels.
#   f32 (wgrad_kernel, 32-pixel chunks): chunks = 82; tiles = ceil(160/64) * 9 * ceil(96/64) = 54;
#     splits = min(ceil(4096 / 54), chunks, 256) = 76, and 82 = 76 + 6: six splits take two chunks;
#   16-bit (wgrad2_kernel, 64-pixel stages): chunks = 41; tiles = ceil(160/64) * ceil(9 * 96 / 64) = 42;
#     splits = min(ceil(4096 / 42) = 98, chunks // 4 = 10, 256) = 10, and 41 = 4 * 10 + 1.
WGRAD_CASES = [(1, 3, 5, 5, 7, 3, 0), (2, 40, 70, 9, 15, 3, 1), (3, 32, 32, 13, 5, 1, 0), (1, 96, 130, 8, 8, 3, 1),
               (1, 64, 64, 5, 13, 3, 1), (2, 96, 130, 32, 41, 3, 1)]
WGRAD_TOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}   # as test_conv_backward_kernels


def _wgrad_plan(n, cin_p, cout_p, ho, wo, k, wide):
    """(splits, chunks) of backward.hip's wgrad2_splits (16-bit operands) / wgrad_splits (f32)."""
    pix = n * ho * wo
    if wide:
        chunks = math.ceil(pix / 64)
        tiles = math.ceil(cout_p / 64) * math.ceil(k * k * cin_p / 64)
        sp = min(math.ceil(4096 / tiles), chunks // 4, 256)
    else:
        chunks = math.ceil(pix / 32)
        tiles = math.ceil(cout_p / 64) * k * k * math.ceil(cin_p / 64)
        sp = min(math.ceil(4096 / tiles), chunks, 256)
    return max(sp, 1), chunks


def test_wgrad_cases_reach_every_path():
    pix = [n * (h + 2 * p - k + 1) * (w + 2 * p - k + 1) for n, _, _, h, w, k, p in WGRAD_CASES]
    assert pix[0] == 15 and pix[3] == 64 and pix[4] == 65      # under one stage, one stage exactly, one pixel more
    assert any(k == 1 for *_, k, _ in WGRAD_CASES) and any(h != w for _, _, _, h, w, _, _ in WGRAD_CASES)
    assert any(ci % 32 and co % 32 for _, ci, co, *_ in WGRAD_CASES)
    n, cin, cout, h, w, k, pad = WGRAD_CASES[-1]
    for wide, expect in ((False, (76, 82)), (True, (10, 41))):
        sp, chunks = _wgrad_plan(n, nv.pad32(cin), nv.pad32(cout), h + 2 * pad - k + 1, w + 2 * pad - k + 1, k, wide)
        assert (sp, chunks) == expect and sp > 1 and chunks % sp != 0


@pytest.fixture(scope="module")
def wgrad_refs():
    """fp64 weight gradients, computed once per (case, dtype) and shared."""
    cache = {}

    def get(case, dtype):
        if (case, dtype) not in cache:
            n, cin, cout, h, w, k, pad = case
            g = _gen(cin * 7 + cout + h)
            x = torch.randn(n, cin, h, w, generator=g).to(dtype)
            dy = torch.randn(n, cout, h + 2 * pad - k + 1, w + 2 * pad - k + 1, generator=g).to(dtype)
            wz = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
            with torch.enable_grad():
                (dw,) = torch.autograd.grad(F.conv2d(x.double(), wz, padding=pad), wz, dy.double())
            cache[(case, dtype)] = (x, dy, dw)
        return cache[(case, dtype)]
    return get


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_wgrad_direct(cuda, wgrad_refs, case, dtype):
    n, cin, cout, h, w, k, pad = case
    cin_p, cout_p = nv.pad32(cin), nv.pad32(cout)
    ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    x, dy, ref = wgrad_refs(case, dtype)
    xd = F.pad(x.permute(0, 2, 3, 1), (0, cin_p - cin)).contiguous().to(cuda)      # NHWC, zero padded
    dyd = F.pad(dy.permute(0, 2, 3, 1), (0, cout_p - cout)).contiguous().to(cuda)
    code, st = nv.dtype_code(dtype), nv.stream_of(xd)
    total = cout_p * k * k * cin_p
    sp = [_wgrad_plan(n, cin_p, cout_p, ho, wo, k, wide)[0] for wide in (False, True)]
    nfl = int(nv.query("ic2_conv_wgrad_ws_floats", n, h, w, cin_p, cout_p, k, k, pad))
    assert nfl == max(sp) * total                              # the plan restated above is the library's
    need = sp[dtype != torch.float32] * total
    ws = Guarded(nfl, torch.float32, cuda)

    # one float too few for this dtype's plan: refused before any launch
    dw_p = Guarded(total, torch.float32, cuda)
    with pytest.raises(RuntimeError, match="workspace too small"):
        nv.call("ic2_conv_wgrad", nv.ptr(xd), nv.ptr(dyd), dw_p.ptr(), code, n, h, w, cin_p, cout_p, k, k, pad, ws.ptr(),
                need - 1, st)
    torch.cuda.synchronize()
    assert bool(_nan_bits(dw_p.t).all()) and bool(_nan_bits(ws.t).all())

    nv.call("ic2_conv_wgrad", nv.ptr(xd), nv.ptr(dyd), dw_p.ptr(), code, n, h, w, cin_p, cout_p, k, k, pad, ws.ptr(), nfl,
            st)
    torch.cuda.synchronize()
    assert dw_p.intact() and ws.intact()
    got_p = dw_p.t.view(cout_p, k, k, cin_p).cpu()
    assert bool(got_p.isfinite().all())                        # the whole padded tensor is written
    assert bool((got_p[..., cin:] == 0).all())                 # x's padded channels are zero
    assert bool((got_p[cout:] == 0).all())                     # ... and dy's
    got = got_p[:cout, :, :, :cin].permute(0, 3, 1, 2).contiguous()
    tol = WGRAD_TOL[dtype]
    rel = ((got.double() - ref).norm() / ref.norm()).item()
    worst = ((got.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"[wgrad {dtype} {case}] relative norm {rel:.2e}, worst element / max|dw| {worst:.2e} (tol {tol:.0e})")
    assert rel < tol
    assert worst < tol                                         # a single wrong tap or channel cannot hide in the norm

    # the nn.Conv2d layout: the same partial sums in the same order, valid channels only, nothing else written
    ws.t.fill_(float("nan"))
    dw_o = Guarded(cout * cin * k * k, torch.float32, cuda)
    with pytest.raises(RuntimeError, match="workspace too small"):
        nv.call("ic2_conv_wgrad_oihw", nv.ptr(xd), nv.ptr(dyd), dw_o.ptr(), code, n, h, w, cin_p, cout_p, cout, cin, k,
                k, pad, ws.ptr(), need - 1, st)
    torch.cuda.synchronize()
    assert bool(_nan_bits(dw_o.t).all())
    nv.call("ic2_conv_wgrad_oihw", nv.ptr(xd), nv.ptr(dyd), dw_o.ptr(), code, n, h, w, cin_p, cout_p, cout, cin, k, k,
            pad, ws.ptr(), nfl, st)
    torch.cuda.synchronize()
    assert dw_o.intact() and ws.intact()
    got_o = dw_o.t.view(cout, cin, k, k).cpu()
    assert bool(got_o.isfinite().all())
    assert _same_bits(got_o, got)


# ================================================================================================ 8. ic2_code_record
def _record(cuda, codes, kind, k, bits, golden, counts=None, times=1):
    """-> counts [k + 2] as uint64 numpy (after `times` calls into the same zeroed counters)."""
    cnt = Guarded(k + 2, torch.int32, cuda, fill=0) if counts is None else counts
    n = codes.numel()
    cd = codes.to(cuda)
    gd = None if golden is None else golden.to(cuda)
    for _ in range(times):
        nv.call("ic2_code_record", nv.ptr(cd), kind, k, bits, nv.ptr(gd), n, cnt.ptr(), nv.stream_of(cd))
    torch.cuda.synchronize()
    assert cnt.intact()
    return cnt.t.cpu().numpy().view(np.uint32).astype(np.uint64)


def _expect_counts(code_i64, valid, k, ndiff):
    """numpy reference: code_i64 where `valid`, everything else in counts[k]."""
    exp = np.zeros(k + 2, dtype=np.uint64)
    exp[:k] = np.bincount(code_i64[valid], minlength=k)
    exp[k] = int((~valid).sum())
    exp[k + 1] = ndiff
    return exp


@pytest.mark.parametrize("k", [2, 256, 8192])                  # 8192: the largest LDS histogram
@pytest.mark.parametrize("n", [1, 255, 4097, 2_200_000])
def test_code_record_indices(cuda, k, n):
    if n > 1_000_000:
        assert math.ceil(n / (256 * 8)) > 1024                 # past the 1024-workgroup cap: the stride loop repeats
    g = _gen(k + n)
    codes = torch.randint(0, k, [n], generator=g, dtype=torch.int64)
    if n >= 255:
        codes[[1, n // 3, n // 2, n - 2]] = torch.tensor([-1, k, 2 ** 40, -2 ** 40])
    golden = codes.clone()
    diff_at = sorted({0, n - 1, n // 2, n // 7})               # the first and the last element among them
    golden[diff_at] += 1
    c = codes.numpy()
    valid = (c >= 0) & (c < k)
    exp = _expect_counts(c, valid, k, len(diff_at))
    assert int(exp[k]) == (4 if n >= 255 else 0)
    got = _record(cuda, codes, 1, k, 0, golden)
    assert int(got[:k].sum() + got[k]) == n
    assert np.array_equal(got, exp)
    assert np.array_equal(_record(cuda, codes, 1, k, 0, golden, times=2), 2 * exp)    # calls accumulate
    exp_nogold = exp.copy()
    exp_nogold[k + 1] = 0
    assert np.array_equal(_record(cuda, codes, 1, k, 0, None), exp_nogold)


@pytest.mark.parametrize("bits", [1, 4, 8, 10])
def test_code_record_latents(cuda, bits):
    k, S = 1 << bits, np.float32((1 << bits) - 1)
    n_grid = 5000
    w = (torch.rand(n_grid, generator=_gen(bits)) * 2 - 1).to(cuda)
    q = torch.empty_like(w)
    nv.call("ic2_quantize_uniform", nv.ptr(w), n_grid, bits, nv.ptr(q), None, nv.stream_of(w))
    one = np.float32(1)
    hand = np.array([-1.0, 1.0, np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2)), 1.5, -1.5, 3.0,
                     -3.0, 0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    codes = torch.cat([torch.from_numpy(hand[:6]), q.cpu(), torch.from_numpy(hand[6:])])   # hand-placed at both ends
    n = codes.numel()
    golden = codes.clone()
    zero_at = n - 5
    assert codes[zero_at].item() == 0.0 and not bool(np.signbit(codes[zero_at].item()))
    golden[zero_at] = -0.0                                      # bitwise comparison: -0.0 differs from +0.0
    golden[0], golden[n // 2] = 0.25, 2.0
    c32 = codes.numpy()
    ndiff = int((c32.view(np.uint32) != golden.numpy().view(np.uint32)).sum())
    assert ndiff == 3                                           # the NaN at n - 1 equals itself bit for bit
    # the documented code, in f32 and in the written order; what is not finite or not in [0, k) is no code
    with np.errstate(invalid="ignore"):
        v = np.rint(((c32 + one) * np.float32(0.5)) * S)
        valid = np.isfinite(v) & (v >= 0) & (v < k)
    exp = _expect_counts(np.where(valid, v, 0).astype(np.int64), valid, k, ndiff)
    assert int(exp[k]) >= 5                                     # +-inf, NaN, +-3.0 at the least
    qi = np.rint((q.cpu().numpy() + one) * np.float32(0.5) * S)
    assert bool(((qi >= 0) & (qi < k)).all())                   # the quantizer's own outputs are all codes
    got = _record(cuda, codes, 0, k, bits, golden)
    assert int(got[:k].sum() + got[k]) == n
    assert np.array_equal(got, exp), (got[:4], exp[:4], got[k:], exp[k:])


def test_code_record_empty_and_invalid(cuda):
    k = 16
    codes = torch.zeros(4, dtype=torch.int64)
    lat = torch.zeros(4)
    cnt = Guarded(8192 + 3, torch.int32, cuda, fill=7)
    before = cnt.t.clone()
    nv.call("ic2_code_record", nv.ptr(codes.to(cuda)), 1, k, 0, None, 0, cnt.ptr(), nv.stream_of(cnt.t))   # n == 0
    for args in ((lat, 0, k, 3), (lat, 0, k, 5), (codes, 1, 8193, 0), (codes, 2, k, 0)):   # k != 2^bits, k > 8192, kind
        src, kind, kk, bits = args
        with pytest.raises(RuntimeError, match="code_record"):
            nv.call("ic2_code_record", nv.ptr(src.to(cuda)), kind, kk, bits, None, 4, cnt.ptr(), nv.stream_of(cnt.t))
    torch.cuda.synchronize()
    assert cnt.intact() and torch.equal(cnt.t, before)
