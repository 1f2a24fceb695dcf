"""GPU: training through the Gumbel-softmax quantizer -- the reference's second trainer,
train_gumbel_discretized_hvae (gumbel_softmax_compression.py:322-611), backpropagates through
GumbelSoftmaxCompressor.forward (:172-200) into the encoder's means and the quantizer's log_temperature.

The reference value is an fp64 restatement of GumbelSoftmaxDiscretization.forward (:93-127) written here and
differentiated by torch autograd; its forward is pinned to oracle.encoder.gumbel_forward (which evaluates in f32, and
is itself pinned to the reference's outputs by tests/golden) to 1e-6.  Bars: 1e-4 relative on dz (norm) and on
dlog tau, the project's fp32 gradient bar (test_encoder_backward_small_fp32); a plain fp32 torch evaluation of the
same formulas sits at <= 4.1e-6, so the bar leaves about 25x for expf / logf and the summation order.

Measured on MI355X (the ten cases of test_kernel_gradient_with_given_noise, w = 0 and 1): worst dz 1.35e-6, worst
dlog tau 7.19e-6; d loss / d means through the whole compressor 1.0e-7.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from image_compression_2_amd import training as ict
from oracle import encoder as oe

pytestmark = pytest.mark.gpu

ENC64 = dict(img_resolution=64, img_channels=3, w_dim=512, num_ws=16, block_split=(5, 12), channel_base=1024,
             channel_max=64)


def _rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def ref64(z, noise, log_t, hard, k):
    """GumbelSoftmaxDiscretization.forward (:93-127) in fp64 with the Gumbel noise given (F.gumbel_softmax's op order:
    (logits + g) / tau, softmax, straight-through one-hot at the argmax when hard) -> (disc [M], perplexity)."""
    cb = torch.linspace(-1, 1, k).float().double()
    d = torch.abs(z.reshape(-1, 1) - cb.reshape(1, -1))
    y = ((-d + noise) / torch.exp(log_t)).softmax(1)
    if hard:
        y = torch.zeros_like(y).scatter_(1, y.max(1, keepdim=True)[1], 1.0) - y.detach() + y
    disc = torch.matmul(y, cb.reshape(-1, 1)).reshape(-1)
    avg = y.mean(0)
    return disc, torch.exp(-torch.sum(avg * torch.log(avg + 1e-10)))


def _latents(m, k, seed):
    """z uniform in [-1.1, 1.1] (some outside the codebook's range), with up to four entries exactly ON codebook
    values (an interior one, the first, the last, another interior one): |z - c| is not differentiable there and
    torch's abs backward uses sign(0) = 0."""
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(m, generator=g) * 2.2 - 1.1
    cb = torch.linspace(-1, 1, k).float()
    for pos, code in zip(dict.fromkeys([0, m // 3, (2 * m) // 3, m - 1]), [k // 3, 0, k - 1, (3 * k) // 4]):
        z[pos] = cb[code]
    noise = oe.gumbel_noise(seed + 1, m, k)
    r = torch.randn(m, generator=g)
    return z, noise, r


GRAD_CASES = [(1, 256, 1.0), (301, 64, 0.5), (301, 100, 0.7), (1023, 256, 0.7), (130, 1024, 0.7)]
_worst = {"dz": 0.0, "dlogt": 0.0}


@pytest.mark.parametrize("m,k,tau", GRAD_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_kernel_gradient_with_given_noise(cuda, hard, m, k, tau):
    """dL/dz and dL/dlog tau of loss = sum(disc * R) + w * perplexity, w in {0, 1}, against fp64 autograd: M not a
    multiple of the 4 waves of a workgroup, a partial lane mask (K = 100), the smallest and the largest K per lane."""
    z, noise, r = _latents(m, k, seed=100 + m + k)
    mod = ic2.GumbelSoftmaxDiscretization(m, k, temperature=tau).to(cuda).train()
    log_t = mod.log_temperature.detach().double().cpu()
    # the restatement's forward is the oracle's (f32) to 1e-6
    with torch.no_grad():
        d64, p64 = ref64(z.double(), noise.double(), log_t, hard, k)
        od, op, _ = oe.gumbel_forward(z, noise, torch.exp(mod.log_temperature.detach().cpu()), hard, n_embeddings=k)
    assert (d64 - od.reshape(-1).double()).abs().max().item() <= 1e-6
    assert abs(p64.item() - op.item()) <= 1e-6 * p64.item()
    fixed = ic2.GumbelSoftmaxDiscretization(m, k, temperature=tau, learnable_temp=False).to(cuda).train()
    for w in (0.0, 1.0):
        zr = z.double().requires_grad_(True)
        lt = log_t.clone().requires_grad_(True)
        d64, p64 = ref64(zr, noise.double(), lt, hard, k)
        ((d64 * r.double()).sum() + w * p64).backward()

        zg = z.to(cuda).view(1, 1, m).requires_grad_(True)
        mod.log_temperature.grad = None
        disc, perp, idx = mod(zg, hard=hard, gumbel_noise=noise.to(cuda))
        assert not idx.requires_grad and disc.requires_grad and perp.requires_grad
        ((disc.view(-1) * r.to(cuda)).sum() + w * perp).backward()
        e_z = _rel(zg.grad, zr.grad)
        e_t = abs(mod.log_temperature.grad.item() - lt.grad.item()) / abs(lt.grad.item())
        _worst["dz"], _worst["dlogt"] = max(_worst["dz"], e_z), max(_worst["dlogt"], e_t)
        print(f"[gumbel-bwd] hard={hard} M={m} K={k} tau={tau} w={w}: dz {e_z:.2e}, dlogtau {e_t:.2e} "
              f"(worst so far: dz {_worst['dz']:.2e}, dlogtau {_worst['dlogt']:.2e})")
        assert zg.grad.shape == zg.shape and zg.grad.dtype == zg.dtype
        assert e_z < 1e-4, e_z
        assert e_t < 1e-4, (mod.log_temperature.grad.item(), lt.grad.item())

        # a fixed temperature (a buffer): no temperature gradient, the same dz
        zf = z.to(cuda).view(1, 1, m).requires_grad_(True)
        disc, perp, _ = fixed(zf, hard=hard, gumbel_noise=noise.to(cuda))
        ((disc.view(-1) * r.to(cuda)).sum() + w * perp).backward()
        assert not fixed.log_temperature.requires_grad and fixed.log_temperature.grad is None
        if w == 0.0 or m <= 4:
            assert torch.equal(zf.grad, zg.grad)
        else:
            # q comes from the forward's column sums, which several workgroups accumulate with float atomics: two
            # forwards agree to the last bits of a k-term f32 sum, not bitwise, and dz inherits that through q
            assert _rel(zf.grad, zg.grad) < 1e-6


def _fwd(z, cb, log_t, hard, seed, noise):
    m, k = z.numel(), cb.numel()
    disc = torch.empty(m, dtype=torch.float32, device=z.device)
    idx = torch.empty(m, dtype=torch.int64, device=z.device)
    nv.call("ic2_gumbel_softmax_quantize_dseed", nv.ptr(z), m, nv.ptr(cb), k, nv.ptr(log_t), 1.0, int(hard),
            nv.ptr(seed), 0, nv.ptr(noise), nv.ptr(disc), nv.ptr(idx), None, nv.stream_of(z))
    return disc, idx


def _bwd(z, cb, log_t, seed, noise, g, q, dz=None, ws=None, dlogt=None):
    m, k = z.numel(), cb.numel()
    nbytes = int(nv.query("ic2_gumbel_softmax_bwd_ws_bytes", m))
    dz = torch.empty(m, dtype=torch.float32, device=z.device) if dz is None else dz
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=z.device) if ws is None else ws
    dlogt = torch.empty(1, dtype=torch.float32, device=z.device) if dlogt is None else dlogt
    assert ws.numel() * 4 == nbytes
    nv.call("ic2_gumbel_softmax_quantize_bwd", nv.ptr(z), m, nv.ptr(cb), k, nv.ptr(log_t), 1.0, nv.ptr(seed), 0,
            nv.ptr(noise), nv.ptr(g), nv.ptr(q), nv.ptr(dz), nv.ptr(dlogt), nv.ptr(ws), nbytes, nv.stream_of(z))
    return dz, dlogt


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_philox_replay(cuda):
    """The backward's in-kernel noise is the forward's: with a fixed device seed and no noise argument, at M = 20,001
    (more than 4 waves x 4096 workgroups: the grid-stride loop runs) and K = 64, the noise dumped by ic2_gumbel_noise
    fed back as gumbel_noise reproduces the generated-noise forward (disc, idx) and backward (dz, dlog tau) bit for
    bit; two backward runs are bit-identical; the dumped noise is Gumbel(0, 1) (mean = Euler's constant)."""
    m, k = 20001, 64
    g = torch.Generator(device=cuda).manual_seed(5)
    z = torch.rand(m, device=cuda, generator=g) * 2.2 - 1.1
    cb = torch.linspace(-1, 1, k).float().to(cuda)
    log_t = torch.full([1], float(np.log(0.7)), device=cuda)
    seed = torch.tensor([0x1234_5678_9ABC_DEF], dtype=torch.int64, device=cuda)
    noise = torch.full([m, k], float("nan"), device=cuda)
    nv.call("ic2_gumbel_noise", nv.ptr(seed), 0, 0, m, k, nv.ptr(noise), nv.stream_of(z))
    by_value = torch.empty_like(noise)   # the seed passed by value: the same stream
    nv.call("ic2_gumbel_noise", None, 0x1234_5678_9ABC_DEF, 0, m, k, nv.ptr(by_value), nv.stream_of(z))
    assert torch.equal(_bits(noise), _bits(by_value))
    assert torch.isfinite(noise).all()
    mean = noise.double().mean().item()
    print(f"[gumbel-noise] mean {mean:.5f} over {m * k} draws")
    assert abs(mean - 0.5772) < 0.01
    for hard in (False, True):
        d_gen, i_gen = _fwd(z, cb, log_t, hard, seed, None)
        d_rep, i_rep = _fwd(z, cb, log_t, hard, None, noise)
        assert torch.equal(_bits(d_gen), _bits(d_rep)) and torch.equal(i_gen, i_rep)
    gup = torch.randn(m, device=cuda, generator=g)
    q = torch.randn(k, device=cuda, generator=g) * 1e-3
    dz_gen, dt_gen = _bwd(z, cb, log_t, seed, None, gup, q)
    dz_rep, dt_rep = _bwd(z, cb, log_t, None, noise, gup, q)
    dz_again, dt_again = _bwd(z, cb, log_t, seed, None, gup, q)
    assert torch.isfinite(dz_gen).all() and torch.isfinite(dt_gen).all() and dz_gen.abs().max() > 0
    assert torch.equal(_bits(dz_gen), _bits(dz_rep)) and torch.equal(_bits(dt_gen), _bits(dt_rep))
    assert torch.equal(_bits(dz_gen), _bits(dz_again)) and torch.equal(_bits(dt_gen), _bits(dt_again))
    other = torch.tensor([7], dtype=torch.int64, device=cuda)   # and the seed matters
    assert not torch.equal(_bits(_bwd(z, cb, log_t, other, None, gup, q)[0]), _bits(dz_gen))


def test_top_philox_draw_gives_finite_noise(cuda):
    """One draw in 2^24 has all of its 24 uniform bits set; (2^24 - 1) + 0.5 rounds to 2^24 in f32, which made
    u = 1, the noise +inf and that latent's softmax NaN -- about two latents per call at the training shape
    (M * K = 2^25), i.e. a NaN perplexity and loss on every step.  For seed 20240607 the Philox4x32-10 counter
    16766590 is such a draw (found with a numpy Philox): the noise there is -log(-log(1 - 2^-24)) = 16.6355, and the
    forward and the backward of the latent that draws it are finite."""
    seed, ctr, k = 20240607, 16766590, 64
    noise = torch.empty(3, device=cuda)
    nv.call("ic2_gumbel_noise", None, seed, ctr - 1, 3, 1, nv.ptr(noise), nv.stream_of(noise))
    print(f"[gumbel-noise] around the top draw: {noise.tolist()}")
    assert torch.isfinite(noise).all()
    assert abs(noise[1].item() - 16.6355) < 1e-3 and noise[0].abs().item() < 10 and noise[2].abs().item() < 10
    z = torch.tensor([0.3, -0.2, 0.9], device=cuda)
    cb = torch.linspace(-1, 1, k).float().to(cuda)
    log_t = torch.zeros(1, device=cuda)
    sd = torch.tensor([seed], dtype=torch.int64, device=cuda)
    offset = ctr - k - 5   # latent 1, entry 5 draws counter `ctr`
    disc = torch.empty(3, device=cuda)
    psum = torch.zeros(k, device=cuda)
    nv.call("ic2_gumbel_softmax_quantize_dseed", nv.ptr(z), 3, nv.ptr(cb), k, nv.ptr(log_t), 1.0, 0, nv.ptr(sd), offset,
            None, nv.ptr(disc), None, nv.ptr(psum), nv.stream_of(z))
    assert torch.isfinite(disc).all() and torch.isfinite(psum).all()
    assert psum[5].item() > 0.99   # the 16.6 outlier takes latent 1's probability mass
    dz = torch.empty(3, device=cuda)
    dlogt = torch.empty(1, device=cuda)
    ws = torch.empty(1, device=cuda)
    gup = torch.ones(3, device=cuda)
    nv.call("ic2_gumbel_softmax_quantize_bwd", nv.ptr(z), 3, nv.ptr(cb), k, nv.ptr(log_t), 1.0, nv.ptr(sd), offset, None,
            nv.ptr(gup), None, nv.ptr(dz), nv.ptr(dlogt), nv.ptr(ws), 4, nv.stream_of(z))
    assert torch.isfinite(dz).all() and torch.isfinite(dlogt).all()


def test_backward_stores_stay_in_bounds(cuda):
    """dz, the workgroup partials and dlog tau are written into views inside sentinel-filled buffers (as
    test_gpu_wino.py's bounds test) at M = 301 (76 workgroups, the last with one latent): every element of the views
    is written, the guard bands are bit-unchanged."""
    m, k, guard, sentinel = 301, 100, 4096, -1234.5
    g = torch.Generator(device=cuda).manual_seed(6)
    z = torch.rand(m, device=cuda, generator=g) * 2.2 - 1.1
    cb = torch.linspace(-1, 1, k).float().to(cuda)
    log_t = torch.zeros(1, device=cuda)
    seed = torch.tensor([11], dtype=torch.int64, device=cuda)
    gup = torch.randn(m, device=cuda, generator=g)
    nws = int(nv.query("ic2_gumbel_softmax_bwd_ws_bytes", m)) // 4
    assert nws == 76
    bufs = {name: torch.full([guard + n + guard], sentinel, device=cuda) for name, n in
            (("dz", m), ("ws", nws), ("dlogt", 1))}
    views = {name: b[guard:b.numel() - guard] for name, b in bufs.items()}
    _bwd(z, cb, log_t, seed, None, gup, None, dz=views["dz"], ws=views["ws"], dlogt=views["dlogt"])
    torch.cuda.synchronize()
    band = torch.full([guard], sentinel, device=cuda)
    for name, b in bufs.items():
        assert torch.equal(_bits(b[:guard]), _bits(band)) and torch.equal(_bits(b[-guard:]), _bits(band)), name
        assert not (views[name] == sentinel).any() and torch.isfinite(views[name]).all(), name
    # the partials are what the finish kernel summed
    assert abs(views["ws"].double().sum().item() - views["dlogt"].item()) <= 1e-6 * views["ws"].abs().sum().item()


def test_non_finite_upstream_gradient_stays_local(cuda):
    """One inf in dL/d disc gives a non-finite dz at that latent (and a non-finite dlog tau) and finite dz everywhere
    else: the f16 loss scaler detects an overflow through this op from the gradients it produces."""
    m, k = 301, 256
    g = torch.Generator(device=cuda).manual_seed(8)
    z = torch.rand(m, device=cuda, generator=g) * 2.2 - 1.1
    cb = torch.linspace(-1, 1, k).float().to(cuda)
    log_t = torch.zeros(1, device=cuda)
    seed = torch.tensor([12], dtype=torch.int64, device=cuda)
    gup = torch.randn(m, device=cuda, generator=g)
    gup[17] = float("inf")
    dz, dlogt = _bwd(z, cb, log_t, seed, None, gup, None)
    finite = torch.isfinite(dz)
    assert not finite[17] and finite.sum().item() == m - 1
    assert not torch.isfinite(dlogt).any()


@pytest.fixture(scope="module")
def gen256_frozen(cuda):
    torch.manual_seed(1)
    G = ic2.Generator(img_resolution=256).to(cuda).eval().requires_grad_(False)
    with torch.no_grad():  # non-unit input gains, as in a trained generator
        for i, L in enumerate(G.synthesis.layers()):
            L.magnitude_ema.fill_(0.6 + 0.05 * i)
    return G


def _compressor(cuda, G):
    torch.manual_seed(0)
    enc = ic2.HVAE_VGG_Encoder(**ENC64).to(cuda)
    return ic2.GumbelSoftmaxCompressor(enc, G, training_resolution=64).to(cuda).train()


def test_compressor_chains_the_quantizer_gradient(cuda, gen256_frozen):
    """compressor(x) in train() mode, loss = MSE + 1e-4 * (perplexity - 256)^2: the gradient that reaches the
    encoder's means equals the fp64 restatement's dz for this call's noise (dumped from this call's seed), chained
    with dL/dw_discrete of the HIP fp32 synthesis + resize + MSE taken on a detached leaf (the synthesis gradient is
    pinned to fp64 in test_gpu_training.py).  log_temperature gets a finite gradient, the frozen generator none."""
    comp = _compressor(cuda, gen256_frozen)
    disc = comp.discretization
    x = (torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    cap = {}

    def keep_means(_mod, _inp, out):
        out[1].retain_grad()
        cap["means"] = out[1]
    hooks = [comp.encoder.register_forward_hook(keep_means),
             disc.register_forward_pre_hook(lambda _m, _i: cap.__setitem__("rng", torch.cuda.get_rng_state(cuda)))]
    try:
        torch.manual_seed(1)
        img, _, w_discrete, perplexity = comp(x)
    finally:
        for h in hooks:
            h.remove()
    loss = F.mse_loss(x, img) + 1e-4 * (perplexity - 256.0) ** 2
    loss.backward()
    means = cap["means"]
    # this call's seed: the quantizer's first draw on the device generator
    after = torch.cuda.get_rng_state(cuda)
    torch.cuda.set_rng_state(cap["rng"], cuda)
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=cuda)
    torch.cuda.set_rng_state(after, cuda)
    m, k = means.numel(), 256
    noise = torch.empty(m, k, device=cuda)
    nv.call("ic2_gumbel_noise", nv.ptr(seed), 0, 0, m, k, nv.ptr(noise), nv.stream_of(noise))
    d_rep, _ = _fwd(means.detach().reshape(-1).contiguous(), disc.codebook, disc.log_temperature.detach(), False, None,
                    noise)
    assert torch.equal(_bits(d_rep), _bits(w_discrete.detach().reshape(-1)))   # the replayed seed is the call's
    # dL_rec/dw_discrete through the fp32 HIP synthesis + resize + MSE on a detached leaf
    wd = w_discrete.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        F.mse_loss(x, ic2.resize_bilinear(gen256_frozen.synthesis(wd), (64, 64))).backward()
    zr = means.detach().double().cpu().reshape(-1).requires_grad_(True)
    lt = disc.log_temperature.detach().double().cpu().requires_grad_(True)
    d64, p64 = ref64(zr, noise.double().cpu(), lt, False, k)
    assert abs(p64.item() - perplexity.item()) < 1e-5 * p64.item()
    ((d64 * wd.grad.double().cpu().reshape(-1)).sum() + 1e-4 * (p64 - 256.0) ** 2).backward()
    err = _rel(means.grad, zr.grad)
    print(f"[gumbel-chain] d loss / d means vs fp64: {err:.2e}; dlogtau {disc.log_temperature.grad.item():.4e} "
          f"(fp64 {lt.grad.item():.4e})")
    assert err < 1e-4
    assert disc.log_temperature.grad is not None and torch.isfinite(disc.log_temperature.grad).all()
    assert all(p.grad is None for p in gen256_frozen.parameters())


def test_train_step_gumbel_updates_encoder_and_temperature(cuda, gen256_frozen):
    comp = _compressor(cuda, gen256_frozen)
    enc, disc = comp.encoder, comp.discretization
    opt = ict.make_gumbel_optimizer(comp, lr=1e-4)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    w_avg = gen256_frozen.mapping.w_avg.view(1, 1, -1)
    with pytest.raises(ValueError, match="perceptual"):
        ict.train_step_gumbel(comp, x, opt, w_avg)
    before = {k: v.detach().clone() for k, v in enc.named_parameters()}
    log_t0, used0 = disc.log_temperature.detach().clone(), disc.usage.sum().item()
    for _ in range(2):
        out = ict.train_step_gumbel(comp, x, opt, w_avg, perceptual_weight=0.0)
    vals = {k: v.item() for k, v in out.items()}
    print(f"[train-step-gumbel] {vals}")
    assert set(vals) == {"rec_loss", "kl_loss", "perceptual_loss", "perplexity_loss", "total_loss", "perplexity"}
    assert all(v.dim() == 0 and v.is_cuda and not v.requires_grad for v in out.values())
    assert all(np.isfinite(v) for v in vals.values()), vals
    total = vals["rec_loss"] + 0.01 * vals["kl_loss"] + 1.0 * vals["perplexity_loss"]
    assert abs(vals["total_loss"] - total) < 1e-5 * abs(total)
    assert abs(vals["perplexity_loss"] - (vals["perplexity"] - 256.0) ** 2) <= 1e-5 * vals["perplexity_loss"] + 1e-12
    assert not torch.equal(disc.log_temperature.detach(), log_t0)
    changed = [k for k, v in enc.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(changed) >= len(before) // 2, changed
    assert disc.usage.sum().item() - used0 == 2 * 2 * 16 * 512
    assert all(p.grad is None for p in gen256_frozen.parameters())


def test_train_step_gumbel_f16_loss_scaler(cuda, gen256_frozen):
    """The reference's fp16 branch (:421, :531, :562-564) as make_f16 + train_step_gumbel(scaler=...): a clean step
    keeps the scale at 2^16 and moves the parameters; a non-finite gradient entering the quantizer's backward reaches
    the scaler through dz and dlog tau, so the step is skipped (parameters and log_temperature bit-unchanged) and the
    scale halves."""
    comp = _compressor(cuda, gen256_frozen)
    enc, disc = comp.encoder, comp.discretization
    opt = ict.make_gumbel_optimizer(comp, lr=1e-4)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    w_avg = gen256_frozen.mapping.w_avg.view(1, 1, -1)
    scaler = ict.make_f16(comp)
    try:
        before = {k: v.detach().clone() for k, v in enc.named_parameters()}
        log_t0 = disc.log_temperature.detach().clone()
        out = ict.train_step_gumbel(comp, x, opt, w_avg, perceptual_weight=0.0, scaler=scaler)
        assert all(np.isfinite(v.item()) for v in out.values()), out
        assert scaler.get_scale() == 65536.0
        changed = [k for k, v in enc.named_parameters() if not torch.equal(v.detach(), before[k])]
        assert len(changed) >= len(before) // 2, changed
        assert not torch.equal(disc.log_temperature.detach(), log_t0)
        # an overflow upstream of the quantizer (the forward re-creates the fine projector's fc1, ref :225-230, so
        # the snapshot is taken after it)
        opt.zero_grad()
        _, means, _ = enc(x)
        snap = {k: v.detach().clone() for k, v in enc.named_parameters()}
        log_t1 = disc.log_temperature.detach().clone()
        w_discrete, _, _ = disc(means)
        poison = torch.ones_like(w_discrete)
        poison[0, 3, 5] = float("inf")
        scaler.scale((w_discrete * poison).sum()).backward()
        assert not torch.isfinite(disc.log_temperature.grad).all()
        scaler.step(opt)
        scaler.update()
        assert scaler.get_scale() == 32768.0
        assert all(torch.equal(v.detach(), snap[k]) for k, v in enc.named_parameters())
        assert torch.equal(disc.log_temperature.detach(), log_t1)
    finally:
        gen256_frozen.set_precision("fp32")
        gen256_frozen.synthesis.train_f16 = False


def test_eval_mode_still_refuses_backward(cuda):
    disc = ic2.GumbelSoftmaxDiscretization(512, 256).to(cuda).eval()
    z = (torch.rand(1, 16, 512, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(cuda)
    d, _, _ = disc(z)
    assert d.requires_grad
    with pytest.raises(nv.AutogradUnsupported):
        d.sum().backward()
    with torch.no_grad():   # and without a graph the training-mode module runs the inference kernel
        d2, _, _ = disc.train()(z)
    assert not d2.requires_grad


def test_quantizer_forward_backward_is_graph_capturable(cuda):
    """The autograd path allocates through torch only and never synchronises: forward + backward of a training-mode
    module captured in a graph replays to the eager run's values (explicit noise, so both see the same draw; the
    forward's atomically accumulated column sums reach the gradients through the perplexity, hence 1e-6 and not
    bitwise)."""
    m, k = 301, 256
    z, noise, r = _latents(m, k, seed=77)
    mod = ic2.GumbelSoftmaxDiscretization(m, k, temperature=0.7).to(cuda).train()
    zg = z.to(cuda).view(1, 1, m).requires_grad_(True)
    noise, r = noise.to(cuda), r.to(cuda)

    def run():
        disc, perp, _ = mod(zg, gumbel_noise=noise)
        return torch.autograd.grad((disc.view(-1) * r).sum() + perp, [zg, mod.log_temperature])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in run()]
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.isfinite(b).all() and _rel(b, a) < 1e-6 for a, b in zip(eager, captured))
