"""GPU: MS-SSIM on the HIP path (ic2_ms_ssim_fwd / ic2_ms_ssim_bwd behind metrics.ms_ssim_terms, uint8_ms_ssim,
ms_ssim, ms_ssim_loss, MSSSIMLoss) against the fp64 restatement tests/ms_ssim_oracle.py (pinned on the CPU in
test_ms_ssim_oracle_host.py), which also derives the bounds used here.

Forward bar, per term:  |got - ref| <= K_FWD * 2^-24 * A,  A the reference's own amplification (oracle docstring).
    derived K (every rounding aligned) 100; measured on the MI355X over the whole table, both modes: 1.46 (typical
    0.1 .. 0.8: roundings are not aligned and a term averages 1 .. 60 000 positions); bar K_FWD = 6, four times
    measured.
Backward bar, per element:  |got - ref| <= K_BWD * 2^-24 * G + EPS,  G the backward chain on error magnitudes.
    derived K 130; measured over noisy and smooth at every shape, three forms: 1.01; bar K_BWD = 6.
    EPS = 1e-30 covers nothing but f32 underflow next to an exactly zero bound.
The value is asserted where every reference term exceeds 0.05, with the terms' bar pushed through
d value / d t_s = w_s value / t_s.  Shapes: the smallest at which the kernels can go wrong (oracle.SHAPES and three
derived from MS_SSIM_TILE), and the workload's 256^2."""
import numpy as np
import pytest
import torch

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from image_compression_2_amd import metrics as icm
from image_compression_2_amd import training as ict

import ms_ssim_oracle as mo

pytestmark = pytest.mark.gpu

K_FWD = 6.0
K_BWD = 6.0
EPS = 1e-30
assert K_FWD < mo.K_FWD_DERIVED and K_BWD < mo.K_BWD_DERIVED

SHAPES = mo.SHAPES + mo.tile_shapes(icm.MS_SSIM_TILE)
_ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _dev(cuda, shape, kind):
    a, b = mo.inputs(shape, kind)
    return a.to(cuda), b.to(cuda)


def _check_terms(got, ref, what):
    assert got.dtype == torch.float64 and got.shape == ref["terms"].shape
    err = (got.cpu() - ref["terms"]).abs()
    ratio = (err / (mo.U * ref["A"])).max().item()
    print(f"[ms-ssim fwd] {what}: max|err| {err.max().item():.3e}  K ratio {ratio:.3f}  terms min "
          f"{ref['terms'].min().item():.4f}")
    assert ratio <= K_FWD, (what, ratio)
    if ref["terms"].min().item() > 0.05:
        value = icm._ms_ssim_value(got).cpu()
        w = torch.tensor(mo.WEIGHTS, dtype=torch.float64)
        per_c = (ref["terms"] ** w).prod(dim=2, keepdim=True)
        bound = (w * per_c / ref["terms"] * K_FWD * mo.U * ref["A"]).sum(dim=2).mean(dim=1)
        verr = (value - ref["value"]).abs()
        print(f"[ms-ssim fwd] {what}: value {ref['value'].tolist()} max|err| {verr.max().item():.3e} "
              f"(bound {bound.min().item():.3e})")
        assert (verr <= bound + 1e-15).all(), (what, verr, bound)


@pytest.mark.parametrize("kind", ["noisy", "smooth", "independent", "negated"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_loss_mode_terms_match_reference(cuda, shape, kind):
    a, b = _dev(cuda, shape, kind)
    _check_terms(icm.ms_ssim_terms(a, b, uint8=False), mo.reference(shape, kind, "loss"), f"loss {shape} {kind}")


@pytest.mark.parametrize("kind", ["noisy", "smooth", "independent", "negated", "clamped"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_metric_mode_terms_match_integer_reference(cuda, shape, kind):
    a, b = _dev(cuda, shape, kind)
    ref = mo.reference(shape, kind, "metric")
    got = icm.ms_ssim_terms(a, b)
    _check_terms(got, ref, f"metric {shape} {kind}")
    per_image = icm.uint8_ms_ssim(a, b)
    assert per_image.dtype == torch.float64 and per_image.shape == (shape[0],)
    assert torch.equal(per_image, icm._ms_ssim_value(got))
    assert icm.ms_ssim(a, b) == sum(per_image.tolist()) / shape[0]


@pytest.mark.parametrize("kind", ["noisy", "clamped"])
@pytest.mark.parametrize("shape", [(1, 3, 163, 189), (2, 3, 256, 256)], ids=_ids)
def test_metric_mode_equals_loss_mode_on_converted_images(cuda, shape, kind):
    """The metric on [-1, 1] inputs against the loss-mode terms of the pre-converted images u/255*2-1: the same
    arithmetic at data range 255 and 1, within the forward bound."""
    a, b = _dev(cuda, shape, kind)
    ref = mo.reference(shape, kind, "metric")
    pre = [(mo.to_uint8(t) / 255.0 * 2 - 1).float().to(cuda) for t in mo.inputs(shape, kind)]
    metric = icm.ms_ssim_terms(a, b)
    loss = icm.ms_ssim_terms(pre[0], pre[1], uint8=False)
    ratio = ((metric - loss).abs().cpu() / (mo.U * ref["A"])).max().item()
    print(f"[ms-ssim fwd] metric vs loss-on-converted {shape} {kind}: K ratio {ratio:.3f}")
    assert ratio <= K_FWD


@pytest.mark.parametrize("shape", [(2, 3, 161, 161), (1, 3, 163, 189), (1, 1, 171, 171), (2, 3, 256, 256)], ids=_ids)
def test_identical_images_give_exactly_one(cuda, shape):
    a = _dev(cuda, shape, "clamped")[0]
    for uint8 in (True, False):
        terms = icm.ms_ssim_terms(a, a.clone(), uint8=uint8)
        assert terms.cpu().tolist() == [[[1.0] * 5] * shape[1]] * shape[0], uint8
    assert icm.uint8_ms_ssim(a, a).tolist() == [1.0] * shape[0] and icm.ms_ssim(a, a) == 1.0
    assert icm.ms_ssim_loss(a, a.clone()).tolist() == [0.0] * shape[0]


def test_planes_do_not_mix_and_runs_are_bitwise_equal(cuda):
    a, b = _dev(cuda, (2, 3, 256, 256), "smooth")
    t2 = icm.ms_ssim_terms(a, b, uint8=False)
    assert torch.equal(t2, icm.ms_ssim_terms(a, b, uint8=False))
    t1 = icm.ms_ssim_terms(a[1:2].clone(), b[1:2].clone(), uint8=False)
    assert torch.equal(t2[1:2], t1)     # an image's partials and their order do not depend on N
    va, vb = a[:, 1:3], b[:, ::2]       # channel-sliced views
    assert not va.is_contiguous()
    assert torch.equal(icm.ms_ssim_terms(va, vb), icm.ms_ssim_terms(va.contiguous(), vb.contiguous()))


def test_small_images_raise_value_error(cuda):
    for shape in ((1, 3, 160, 256), (1, 3, 256, 160), (2, 3, 64, 64)):
        x = torch.zeros(shape, device=cuda)
        for fn in (icm.ms_ssim_terms, icm.uint8_ms_ssim, icm.ms_ssim, icm.ms_ssim_loss):
            with pytest.raises(ValueError, match="160"):
                fn(x, x)
    with pytest.raises(ValueError):
        icm.ms_ssim_terms(torch.zeros(1, 3, 161, 161, device=cuda), torch.zeros(1, 3, 161, 162, device=cuda))


# ------------------------------------------------------------------------------------------------ backward
def _loss_grads(a, b, up, form):
    a = a.clone().requires_grad_(form in ("a", "both"))
    b = b.clone().requires_grad_(form in ("b", "both"))
    loss = icm.ms_ssim_loss(a, b)
    assert loss.dtype == torch.float32 and loss.shape == (a.shape[0],)
    (loss * up.to(loss.device, torch.float32)).sum().backward()
    return loss.detach(), a.grad, b.grad


def _check_grad(got, ref, G, what):
    err = (got.double().cpu() - ref).abs()
    ratio = (err / (mo.U * G + EPS / K_BWD)).max().item()
    print(f"[ms-ssim bwd] {what}: max|g| {ref.abs().max().item():.3e} max|err| {err.max().item():.3e} "
          f"K ratio {ratio:.3f}")
    assert torch.isfinite(got).all()
    assert ratio <= K_BWD, (what, ratio)


@pytest.mark.parametrize("form", ["a", "b", "both"])
@pytest.mark.parametrize("kind", ["noisy", "smooth"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gradients_match_fp64_autograd(cuda, shape, kind, form):
    a, b = _dev(cuda, shape, kind)
    r = mo.reference_grads(shape, kind)
    loss, ga, gb = _loss_grads(a, b, mo.upstream_of(shape[0]), form)
    assert (loss.double().cpu() - r["loss"]).abs().max().item() <= 1e-6   # f32 output of a value near 0.003 .. 0.02
    assert (ga is None) == (form == "b") and (gb is None) == (form == "a")
    if ga is not None:
        _check_grad(ga, r["ga"], r["Ga"], f"{shape} {kind} d/da ({form})")
    if gb is not None:
        _check_grad(gb, r["gb"], r["Gb"], f"{shape} {kind} d/db ({form})")


@pytest.mark.parametrize("shape", [(1, 3, 163, 189), (2, 3, 161, 161)], ids=_ids)
def test_negated_images_have_zero_gradient(cuda, shape):
    a, b = _dev(cuda, shape, "negated")
    loss, ga, gb = _loss_grads(a, b, mo.upstream_of(shape[0]), "both")
    assert loss.tolist() == [1.0] * shape[0]
    for g in (ga, gb):
        assert torch.isfinite(g).all() and not g.any()


def test_zero_gradient_image_leaves_its_neighbour_alone(cuda):
    shape = (1, 3, 163, 189)
    na, nb = _dev(cuda, shape, "negated")
    sa, sb = _dev(cuda, shape, "smooth")
    up = torch.tensor([0.7, 1.6], dtype=torch.float64)
    loss2, ga2, gb2 = _loss_grads(torch.cat([na, sa]), torch.cat([nb, sb]), up, "both")
    loss1, ga1, gb1 = _loss_grads(sa, sb, up[1:], "both")
    assert loss2[0].item() == 1.0 and loss2[1].item() == loss1[0].item()
    assert not ga2[0].any() and not gb2[0].any()
    assert torch.equal(ga2[1], ga1[0]) and torch.equal(gb2[1], gb1[0])


def test_replicated_planes_keep_their_own_weights(cuda):
    """One 161 x 161 plane replicated to n * c = 96 planes, each with its own upstream weight: every plane's terms are
    plane 0's bit for bit, and every plane's gradient is the oracle's times its weight (a row, a partial or a pooled
    level taken from a neighbouring plane is off by a factor)."""
    shape = (1, 1, 161, 161)
    a1, b1 = mo.inputs(shape, "smooth")
    r = mo.reference_grads(shape, "smooth")
    n, c = 32, 3
    a = a1.expand(n, c, 161, 161).contiguous().to(cuda)
    b = b1.expand(n, c, 161, 161).contiguous().to(cuda)
    terms, ws = icm._ms_ssim_forward(a, b, 0)
    assert torch.equal(terms, terms[:1, :1].expand(n, c, 5))
    base = mo.gterms_of(r["terms"], mo.upstream_of(1))[0, 0]                     # [5], of upstream_of(1)
    weight = 0.25 + torch.arange(n * c, dtype=torch.float64).view(n, c, 1) * 0.125    # exact in f32
    gterms = (base.view(1, 1, 5) * weight).contiguous().to(cuda)
    ga, gb = torch.empty_like(a), torch.empty_like(b)
    ws_grad = torch.empty(int(nv.query("ic2_ms_ssim_bwd_ws_floats", n, c, 161, 161)), device=cuda)
    nv.call("ic2_ms_ssim_bwd", nv.ptr(a), nv.ptr(b), 0, nv.ptr(ws), nv.ptr(gterms), n, c, 161, 161, nv.ptr(ga),
            nv.ptr(gb), nv.ptr(ws_grad), nv.stream_of(a))
    wv = weight.view(n, c, 1, 1)
    for got, ref, G, name in ((ga, r["ga"], r["Ga"], "a"), (gb, r["gb"], r["Gb"], "b")):
        err = (got.double().cpu() - ref * wv).abs()
        ratio = (err / (mo.U * G * wv + EPS)).amax(dim=(2, 3))
        print(f"[ms-ssim bwd] replicated d/d{name}: worst K ratio {ratio.max().item():.3f} at plane "
              f"{ratio.argmax().item()}")
        assert ratio.max().item() <= K_BWD


def test_double_backward_is_refused(cuda):
    a, b = _dev(cuda, (1, 1, 161, 200), "noisy")
    b = b.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(icm.ms_ssim_loss(a, b).sum(), b, create_graph=True)
    assert g.requires_grad
    with pytest.raises(nv.AutogradUnsupported, match="double backward"):
        g.sum().backward()


def test_forward_and_backward_replay_from_a_graph(cuda):
    """ic2_ms_ssim_fwd and ic2_ms_ssim_bwd on caller-owned buffers, captured in one graph and replayed twice: terms and
    both gradients are bit-identical to the eager calls (the entry points neither allocate nor synchronise, and the
    reductions have a fixed order)."""
    shape = (1, 3, 163, 189)
    n, c, h, w = shape
    a, b = _dev(cuda, shape, "smooth")
    gterms = mo.gterms_of(mo.reference_grads(shape, "smooth")["terms"], mo.upstream_of(n)).contiguous().to(cuda)
    ws_floats = int(nv.query("ic2_ms_ssim_ws_floats", n, c, h, w))
    ws_grad_floats = int(nv.query("ic2_ms_ssim_bwd_ws_floats", n, c, h, w))

    def buffers():
        return (torch.zeros(n, c, 5, dtype=torch.float64, device=cuda),
                torch.zeros((ws_floats + 1) // 2, dtype=torch.float64, device=cuda), torch.zeros_like(a),
                torch.zeros_like(b), torch.zeros(ws_grad_floats, device=cuda))

    def run(terms, ws, ga, gb, ws_grad, stream):
        nv.call("ic2_ms_ssim_fwd", nv.ptr(a), nv.ptr(b), 0, n, c, h, w, nv.ptr(terms), nv.ptr(ws), stream)
        nv.call("ic2_ms_ssim_bwd", nv.ptr(a), nv.ptr(b), 0, nv.ptr(ws), nv.ptr(gterms), n, c, h, w, nv.ptr(ga),
                nv.ptr(gb), nv.ptr(ws_grad), stream)
    eager = buffers()
    run(*eager, nv.stream_of(a))
    captured = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(*captured, nv.stream_of(a))
    assert not captured[0].any() and not captured[2].any()      # capturing launched nothing
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for i in (0, 2, 3):
            assert torch.equal(captured[i], eager[i]), i
    assert torch.equal(eager[0], icm.ms_ssim_terms(a, b, uint8=False))


def test_python_layer_refuses_to_run_inside_a_graph_capture(cuda, monkeypatch):
    """The Python layer is not capturable (metrics._ms_refuse_capture): with the current stream reported as capturing,
    every public function raises before anything is launched, the backward of a loss taken outside included.  (No
    capture is begun here: the query is patched, so nothing has to end a capture after an exception.)"""
    a, b = _dev(cuda, (1, 1, 161, 200), "noisy")
    b = b.clone().requires_grad_(True)
    loss = icm.ms_ssim_loss(a, b)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for fn in (icm.ms_ssim_terms, icm.uint8_ms_ssim, icm.ms_ssim, icm.ms_ssim_loss, ic2.MSSSIMLoss()):
        with pytest.raises(RuntimeError, match="graph capture"):
            fn(a, b)
        with pytest.raises(RuntimeError, match="graph capture"):
            fn(a.half(), b.detach())
    with pytest.raises(RuntimeError, match="graph capture"):
        loss.sum().backward()
    assert b.grad is None
    monkeypatch.undo()
    icm.ms_ssim_loss(a, b).sum().backward()
    assert b.grad is not None and torch.isfinite(b.grad).all()


# ------------------------------------------------------------------------------------------------ training
ENC64 = dict(img_resolution=64, img_channels=3, w_dim=512, num_ws=16, block_split=(5, 12), channel_base=1024,
             channel_max=64)


@pytest.fixture(scope="module")
def gen256_frozen(cuda):
    torch.manual_seed(1)
    return ic2.Generator(img_resolution=256).to(cuda).eval().requires_grad_(False)


def _train_grads(cuda, G, prec, weight, percep):
    x = (torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    w_avg = G.mapping.w_avg.view(1, 1, -1)
    torch.manual_seed(0)
    enc = ic2.HVAE_VGG_Encoder(**ENC64).to(cuda)
    comp = ic2.StyleGAN3Compressor(enc, G, training_resolution=None)
    opt = ict.make_optimizer(enc, lr=1e-4)
    scaler = ict.make_f16(comp) if prec == "f16" else None
    try:
        torch.manual_seed(3)
        out = ict.train_step(comp, x, opt, w_avg, perceptual_weight=weight, percep=percep, scaler=scaler)
    finally:
        G.set_precision("fp32")
        G.synthesis.train_f16 = False
    return out, {k: v.grad.detach().clone() for k, v in enc.named_parameters() if v.grad is not None}, enc


@pytest.mark.parametrize("prec", ["fp32", "f16"])
def test_train_step_with_ms_ssim_perceptual_term(cuda, gen256_frozen, prec):
    out0, g0, _ = _train_grads(cuda, gen256_frozen, prec, 0.0, None)
    out, g, enc = _train_grads(cuda, gen256_frozen, prec, 0.8, ic2.MSSSIMLoss())
    vals = {k: v.item() for k, v in out.items()}
    print(f"[train-step ms-ssim {prec}] {vals}")
    assert all(np.isfinite(v) for v in vals.values()), vals
    assert 0.0 < vals["perceptual_loss"] < 1.0 and out0["perceptual_loss"].item() == 0.0
    total = vals["rec_loss"] + 0.8 * vals["perceptual_loss"] + 0.01 * vals["kl_loss"]
    if prec == "fp32":
        assert abs(vals["total_loss"] - total) < 1e-5 * abs(total)
    names = [k for k, _ in enc.named_parameters()]
    assert sorted(g) == sorted(names) == sorted(g0)
    assert all(torch.isfinite(v).all() for v in g.values())
    differing = [k for k in names if not torch.equal(g[k], g0[k])]
    assert len(differing) >= len(names) // 2, differing
    assert all(p.grad is None for p in gen256_frozen.parameters())


def test_image_gradient_through_the_loss_as_train_step_takes_it(cuda):
    """percep(images, reconstructed).mean() with only the reconstruction requiring a gradient."""
    shape = (2, 3, 161, 161)
    a, b = _dev(cuda, shape, "smooth")
    b = b.clone().requires_grad_(True)
    ic2.MSSSIMLoss()(a, b).mean().backward()
    a64, b64 = mo.inputs(shape, "smooth")
    up = torch.full((2,), 0.5, dtype=torch.float64)
    _, terms, _, gb = mo.loss_and_grads(a64, b64, up)
    _, Gb = mo.grad_bound(a64, b64, mo.gterms_of(terms, up))
    _check_grad(b.grad, gb, Gb, "MSSSIMLoss().mean() d/d reconstructed")


def test_train_step_gumbel_accepts_the_same_callable(cuda, gen256_frozen):
    torch.manual_seed(0)
    enc = ic2.HVAE_VGG_Encoder(**ENC64).to(cuda)
    comp = ic2.GumbelSoftmaxCompressor(enc, gen256_frozen, training_resolution=None).to(cuda).train()
    opt = ict.make_gumbel_optimizer(comp, lr=1e-4)
    x = (torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    out = ict.train_step_gumbel(comp, x, opt, gen256_frozen.mapping.w_avg.view(1, 1, -1), percep=ic2.MSSSIMLoss())
    vals = {k: v.item() for k, v in out.items()}
    assert all(np.isfinite(v) for v in vals.values()), vals
    assert 0.0 < vals["perceptual_loss"] < 1.0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in enc.parameters())


# ------------------------------------------------------------------------------------------------ evaluation record
def test_evaluate_compression_ms_ssim_is_opt_in(cuda, gen256_frozen):
    torch.manual_seed(7)
    enc = ic2.HVAE_VGG_Encoder(img_resolution=64, channel_base=256, channel_max=32).to(cuda)
    comp = ic2.StyleGAN3Compressor(enc, gen256_frozen, training_resolution=None)
    x = (torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    torch.manual_seed(3)
    plain = ic2.evaluate_compression(comp, x)
    assert set(plain) == {"original_size_bytes", "compressed_size_bytes", "compression_ratio", "bpp", "psnr_no_quant",
                          "ssim_no_quant", "psnr_quantized", "ssim_quantized", "batch_psnr_no_quant",
                          "batch_ssim_no_quant", "batch_psnr_quantized", "batch_ssim_quantized", "n_images"}
    torch.manual_seed(3)
    rec = ic2.evaluate_compression(comp, x, ms_ssim=True)
    extra = {"ms_ssim_no_quant", "ms_ssim_quantized", "batch_ms_ssim_no_quant", "batch_ms_ssim_quantized"}
    assert set(rec) == set(plain) | extra
    assert {k: rec[k] for k in plain} == plain
    # the record's call sequence from the same seed (the encoder redraws the fine projector's fc1 on every call)
    torch.manual_seed(3)
    with torch.no_grad():
        rn, _ = comp(x)
        rq = comp.decompress(comp.compress(x, 8))
    assert rec["ms_ssim_no_quant"] == icm.uint8_ms_ssim(rn, x).tolist()
    assert rec["ms_ssim_quantized"] == icm.uint8_ms_ssim(rq, x).tolist()
    assert len(rec["ms_ssim_no_quant"]) == 2 and all(0.0 <= v <= 1.0 for v in rec["ms_ssim_no_quant"])
    for name in ("no_quant", "quantized"):
        assert rec["batch_ms_ssim_" + name] == pytest.approx(sum(rec["ms_ssim_" + name]) / 2, abs=1e-15)
    torch.manual_seed(3)
    assert ic2.evaluate_compression(comp, x, ms_ssim=True, reduce=True) == rec
