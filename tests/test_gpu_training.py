"""GPU: the training path's backward (BASELINE C5; reference train_hvae_encoder, stylegan3_hvae_full.py:655-707)
against torch.autograd through the fp64 oracle encoder (oracle/encoder.py, pinned to the reference's own
encoder by tests/golden): every parameter gradient and the input gradient, fp32 mode at the reference's
small golden config and at the full 1024-config on 256^2; bf16 mode within a relative-norm bound; plus the
individual backward kernels against torch on random shapes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from image_compression_2_amd import autograd_ops as ao
from oracle import encoder as oe

pytestmark = pytest.mark.gpu

SMALL = dict(img_resolution=64, img_channels=3, w_dim=32, num_ws=16, block_split=(5, 12), channel_base=256,
             channel_max=32)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _grad_check(cuda, kw, x, precision, tol, seed=7, loss_scale=1.0):
    torch.manual_seed(seed)
    enc = ic2.HVAE_VGG_Encoder(precision=precision, **kw).to(cuda)
    xg = x.clone().to(cuda).requires_grad_(True)
    torch.manual_seed(seed + 1)
    w, m, lv = enc(xg)
    g = torch.Generator().manual_seed(3)
    r = [torch.randn(t.shape, generator=g) for t in (w, m, lv)]
    loss = sum((t * ri.to(cuda)).sum() for t, ri in zip((w, m, lv), r))
    (loss * loss_scale).backward()   # f16: scaled as the reference's GradScaler scales its loss
    # oracle: same weights (fp64 leaves), the fc1 this call drew, the eps this call drew
    named = dict(enc.named_parameters())
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in named.items()}
    fc1 = (sd["fine_projector.fc1.weight"], sd["fine_projector.fc1.bias"])
    eps_all = ((w - m) / torch.exp(0.5 * lv)).detach().cpu().double()
    nws = kw.get("num_ws", 16)
    bs = kw.get("block_split", (5, 12))
    eps = {"global": eps_all[:, :bs[0]], "medium": eps_all[:, bs[0]:bs[1]], "fine": eps_all[:, bs[1]:nws]}
    x64 = x.double().requires_grad_(True)
    ow, om, olv = oe.encoder_forward(sd, x64, num_ws=nws, block_split=bs, w_dim=kw.get("w_dim", 512), fine_fc1=fc1,
                                     eps=eps)
    oloss = sum((t * ri.double()).sum() for t, ri in zip((ow, om, olv), r))
    oloss.backward()
    pairs = {k: (p.grad, sd[k].grad) for k, p in named.items() if sd[k].grad is not None}
    for k, p in named.items():
        if sd[k].grad is None:  # blocks past the reference's 1x1 break (:129-131) take no part, in both
            assert p.grad is None, k
    pairs["x"] = (xg.grad, x64.grad)
    for k, (a, b) in pairs.items():
        assert a is not None, k
    gmax = max(b.norm().item() for _, b in pairs.values())
    worst = {}
    for k, (a, b) in pairs.items():
        a = a.detach().double().cpu() / loss_scale
        if b.norm().item() < 1e-8 * gmax:
            # exactly-zero true gradient (conv bias before a one-channel GroupNorm group): rounding noise only
            assert a.norm().item() < 1e-4 * gmax, k
            continue
        worst[k] = ((a - b).norm() / b.norm()).item()
    bad = {k: v for k, v in worst.items() if v > tol}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f"[train-{precision}] max relative grad error {max(worst.values()):.2e} over {len(worst)} tensors; "
          f"largest: {[(k, round(v, 4)) for k, v in top]}")
    assert not bad, bad


def test_encoder_backward_small_fp32(cuda):
    x = torch.rand(3, 3, 32, 32, generator=torch.Generator().manual_seed(8)) * 2 - 1
    _grad_check(cuda, SMALL, x, "fp32", 1e-4)


def test_encoder_backward_full_fp32(cuda):
    """HVAE_VGG_Encoder(img_resolution=1024) on 256^2 (blocks 0-7 run, 8-9 skipped as in the reference)."""
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(1)) * 2 - 1
    _grad_check(cuda, dict(img_resolution=1024), x, "fp32", 1e-3, seed=0)


def test_encoder_backward_full_f16(cuda):
    """f16 mode, BASELINE config 5's precision (the reference's fp16 autocast + GradScaler, stylegan3_hvae_full.py:
    487,669,693-696): f16 activations, gradients and MFMA operands, f32 accumulation and weight gradients, the loss
    scaled by 2^10 before backward and the gradients unscaled after, as the scaler does.  11-bit significands: the
    same GroupNorm amplification as bf16 (below) at ~1/8 of its error."""
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(1)) * 2 - 1
    # measured on MI355X: 0.070 on the input gradient (from_rgb's 3-channel dgrad: a cancelling sum over 32 channels),
    # <= 0.035 on every parameter (bf16: 0.19)
    _grad_check(cuda, dict(img_resolution=1024), x, "f16", 0.12, seed=0, loss_scale=1024.0)


def test_encoder_backward_full_bf16(cuda):
    """bf16 mode (activations, dy and MFMA operands in bf16; f32 accumulation and weight gradients).  The
    GroupNorm backward of the 8^2 .. 2^2 blocks (16 channels x <= 64 pixels per group) amplifies the bf16
    rounding of the pre-norm activations: measured <= 0.19 relative error there, 0.02-0.05 in the wide blocks
    (a wrong kernel shows O(1))."""
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(1)) * 2 - 1
    _grad_check(cuda, dict(img_resolution=1024), x, "bf16", 0.25, seed=0)


@pytest.mark.parametrize("cin,cout,size,pad,n", [(3, 32, 17, 1, 2), (32, 64, 20, 1, 3), (64, 96, 9, 1, 2),
                                                 (128, 32, 11, 2, 1), (96, 128, 13, 0, 2)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_conv_backward_kernels(cuda, cin, cout, size, pad, n, dtype):
    """Conv2dNHWC backward (dx: the implicit GEMM on flipped / transposed weights; dW: ic2_conv_wgrad with the
    32-pixel K chunks split over workgroups; db) against torch autograd in fp64 on the same (rounded) operands."""
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn(n, cin, size, size, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    b = torch.randn(cout, generator=g)
    dy = torch.randn(n, cout, size + 2 * pad - 2, size + 2 * pad - 2, generator=g)
    cin_p, cout_p = nv.pad32(cin), nv.pad32(cout)
    xd = ao.ToNHWC.apply(x.to(cuda), dtype, cin_p).detach().requires_grad_(True)
    wd, bd = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    with torch.enable_grad():
        y = ao.Conv2dNHWC.apply(xd, wd, bd, pad, cout_p)
        dyd = F.pad(dy.permute(0, 2, 3, 1), (0, cout_p - cout)).to(cuda, dtype)
        y.backward(dyd)
    xr = x.to(dtype).double().requires_grad_(True)
    wr = w.to(dtype).double().requires_grad_(True) if dtype != torch.float32 else w.double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    F.conv2d(xr, wr, br, padding=pad).backward(dy.to(dtype).double())
    tol = {torch.float32: 1e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}[dtype]
    dx = xd.grad.float().cpu()[..., :cin].permute(0, 3, 1, 2)
    assert _rel(dx, xr.grad) < tol
    assert xd.grad.float()[..., cin:].abs().max().item() == 0.0 if cin < cin_p else True
    assert _rel(wd.grad, wr.grad) < tol
    assert _rel(bd.grad, br.grad) < tol


@pytest.mark.parametrize("cin,cout,h,w,pad,n", [(40, 70, 9, 15, 1, 2), (32, 64, 13, 5, 0, 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_conv_backward_kernels_nonsquare(cuda, cin, cout, h, w, pad, n, dtype):
    """The same check with h != w (a swapped height / width in the data gradient's geometry passes every square
    case), and with cin < cin_p and cout < cout_p together."""
    g = torch.Generator().manual_seed(cin * 7 + cout + h)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    b = torch.randn(cout, generator=g)
    dy = torch.randn(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, generator=g)
    cin_p, cout_p = nv.pad32(cin), nv.pad32(cout)
    xd = ao.ToNHWC.apply(x.to(cuda), dtype, cin_p).detach().requires_grad_(True)
    wd, bd = wt.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    with torch.enable_grad():
        y = ao.Conv2dNHWC.apply(xd, wd, bd, pad, cout_p)
        assert y.shape == (n, h + 2 * pad - 2, w + 2 * pad - 2, cout_p)
        y.backward(F.pad(dy.permute(0, 2, 3, 1), (0, cout_p - cout)).to(cuda, dtype))
    xr = x.to(dtype).double().requires_grad_(True)
    wr = wt.to(dtype).double().requires_grad_(True) if dtype != torch.float32 else wt.double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    F.conv2d(xr, wr, br, padding=pad).backward(dy.to(dtype).double())
    tol = {torch.float32: 1e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}[dtype]
    assert xd.grad.shape == (n, h, w, cin_p)
    assert _rel(xd.grad.float().cpu()[..., :cin].permute(0, 3, 1, 2), xr.grad) < tol
    if cin < cin_p:
        assert xd.grad.float()[..., cin:].abs().max().item() == 0.0
    assert _rel(wd.grad, wr.grad) < tol
    assert _rel(bd.grad, br.grad) < tol


@pytest.mark.parametrize("n,c,groups,h,w,pool", [(2, 64, 32, 6, 8, True), (3, 32, 32, 9, 7, False),
                                                 (2, 128, 32, 5, 5, True), (1, 512, 32, 2, 2, True),
                                                 (2, 96, 32, 33, 17, False)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_group_norm_backward_kernel(cuda, n, c, groups, h, w, pool, dtype):
    g = torch.Generator().manual_seed(c + h)
    y = torch.randn(n, c, h, w, generator=g) * 2 + 0.3
    gam = torch.rand(c, generator=g) + 0.5
    bet = torch.randn(c, generator=g) * 0.3
    c_p = nv.pad32(c)
    yd = ao.ToNHWC.apply(y.to(cuda), dtype, c_p).detach().requires_grad_(True)
    gd, bd = gam.to(cuda).requires_grad_(True), bet.to(cuda).requires_grad_(True)
    with torch.enable_grad():
        out = ao.GroupNormLReluPoolNHWC.apply(yd, gd, bd, groups, 1e-5, 0.2, pool, c, dtype)
        dout = torch.randn(out.shape[0], out.shape[1], out.shape[2], c, generator=g)
        out.backward(F.pad(dout, (0, c_p - c)).to(cuda, dtype))
    yr = y.to(dtype).double().requires_grad_(True)
    gr, br = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    o = F.leaky_relu(F.group_norm(yr, groups, gr, br, 1e-5), 0.2)
    if pool:
        o = F.avg_pool2d(o, 2, 2)
    o.backward(dout.to(dtype).double().permute(0, 3, 1, 2))
    tol = {torch.float32: 1e-4, torch.bfloat16: 3e-2, torch.float16: 4e-3}[dtype]
    assert _rel(yd.grad.float().cpu()[..., :c].permute(0, 3, 1, 2), yr.grad) < tol
    assert _rel(gd.grad, gr.grad) < tol and _rel(bd.grad, br.grad) < tol
    # the producing conv's bias gradient from the same call (ic2_gn_lrelu_pool_bwd_db's dsum, f64 channel sums):
    # sum over (n, p) of dy, against the fp64 reference and the column sum of the dy it stored
    yn = ao.ToNHWC.apply(y.to(cuda), dtype, c_p).contiguous()
    nfl = int(nv.query("ic2_group_norm_stats_floats", n, h * w, groups))
    stats = torch.empty([nfl], dtype=torch.float32, device=cuda)
    st = nv.stream_of(yn)
    nv.call("ic2_group_norm_stats", nv.ptr(yn), nv.dtype_code(dtype), n, h * w, c_p, c, groups, 1e-5, nv.ptr(stats),
            st)
    dn = F.pad(dout, (0, c_p - c)).to(cuda, dtype).contiguous()
    wsf = int(nv.query("ic2_gn_lrelu_pool_bwd_floats", n, h, w, c_p, groups))
    ws = torch.empty([wsf], dtype=torch.float32, device=cuda)
    dy = torch.empty_like(yn)
    dsum = torch.empty([c], dtype=torch.float32, device=cuda)
    g32, b32 = gam.to(cuda), bet.to(cuda)
    nv.call("ic2_gn_lrelu_pool_bwd_db", nv.ptr(yn), nv.ptr(dn), nv.ptr(dy), nv.dtype_code(dtype), nv.dtype_code(dtype),
            nv.dtype_code(dtype), n, h, w, c_p, c, groups, nv.ptr(stats), nv.ptr(g32), nv.ptr(b32), 0.2, int(pool), None,
            None, nv.ptr(dsum), nv.ptr(ws), wsf, st)
    # (with one channel per group the per-channel sum is exactly 0: bound the error by the size of the terms)
    ref_sum = yr.grad.sum(dim=(0, 2, 3))
    scale = float(yr.grad.abs().sum(dim=(0, 2, 3)).max())
    assert float((dsum.cpu().double() - ref_sum).abs().max()) < tol * scale
    assert float((dsum.double() - dy.float()[..., :c].sum(dim=(0, 1, 2)).double()).abs().max()) < tol * scale


# ================================================================ synthesis backward (the frozen generator)
@pytest.mark.parametrize("cout,cin,k,dt", [(64, 32, 3, torch.float16), (130, 96, 3, torch.bfloat16),
                                            (40, 3, 3, torch.float32), (16, 24, 1, torch.float16)])
def test_pack_weight_adjoint_equals_flip_transpose_pack(cuda, cout, cin, k, dt):
    """ic2_pack_weight_adjoint (the dgrad pack gathered in one launch) equals ic2_pack_weight on the torch-flipped,
    channel-transposed weight, bit for bit, padding included."""
    w = torch.randn(cout, cin, k, k, device=cuda, generator=torch.Generator(device=cuda).manual_seed(cout + cin))
    cout_p, cin_p = nv.pad32(cout), nv.pad32(cin)
    got = ao.pack_conv_weight_adjoint(w, cout_p, cin_p, dt)
    ref = ao.pack_conv_weight(w.transpose(0, 1).flip(2, 3), cout_p, cin_p, dt)
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (cin_p, k, k, cout_p)
    assert torch.equal(got.view(torch.int16) if dt != torch.float32 else got,
                       ref.view(torch.int16) if dt != torch.float32 else ref)


from image_compression_2_amd import sg3_ops  # noqa: E402
from image_compression_2_amd import training as ict  # noqa: E402
from oracle import sg3  # noqa: E402


def _sd64(module):
    return {k: v.detach().double().cpu() for k, v in module.state_dict().items()}


@pytest.fixture(scope="module")
def gen256_frozen(cuda):
    torch.manual_seed(1)
    G = ic2.Generator(img_resolution=256).to(cuda).eval().requires_grad_(False)
    with torch.no_grad():  # non-unit input gains, as in a trained generator
        for i, L in enumerate(G.synthesis.layers()):
            L.magnitude_ema.fill_(0.6 + 0.05 * i)
    return G


@pytest.mark.parametrize("h,w,taps,up,down,pad,flip", [(12, 14, 12, 2, 1, [7, 6, 7, 6], False),
                                                       (30, 30, 12, 1, 2, 0, False),
                                                       (9, 11, 24, 4, 1, [13, 11, 14, 10], True),
                                                       (10, 10, 5, 2, 2, [1, 3, 2, 0], False)])
def test_sg3_upfirdn2d_gradient(cuda, h, w, taps, up, down, pad, flip):
    g = torch.Generator().manual_seed(taps + h)
    x = torch.randn(2, 5, h, w, generator=g)
    f = torch.rand(taps, generator=g) + 0.1
    xd = x.to(cuda).requires_grad_(True)
    y = sg3_ops.upfirdn2d(xd, f.to(cuda), up=up, down=down, padding=pad, flip_filter=flip, gain=up * up)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.to(cuda))
    xr = x.double().requires_grad_(True)
    sg3.upfirdn2d(xr, f.double(), up=up, down=down, padding=pad, flip_filter=flip, gain=up * up).backward(dy.double())
    assert _rel(xd.grad, xr.grad) < 1e-5


@pytest.mark.parametrize("act,clamp", [("lrelu", 1.0), ("linear", 0.5), ("lrelu", None)])
def test_sg3_bias_act_gradient(cuda, act, clamp):
    g = torch.Generator().manual_seed(11)
    x, b = torch.randn(3, 7, 9, 9, generator=g), torch.randn(7, generator=g) * 0.3
    xd, bd = x.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    y = sg3_ops.bias_act(xd, bd, act=act, clamp=clamp)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.to(cuda))
    xr, br = x.double().requires_grad_(True), b.double().requires_grad_(True)
    sg3.bias_act(xr, br, act=act, clamp=clamp).backward(dy.double())
    assert _rel(xd.grad, xr.grad) < 1e-6 and _rel(bd.grad, br.grad) < 1e-6


@pytest.mark.parametrize("li", [2, 5, 12])
def test_sg3_filtered_lrelu_gradient(cuda, li):
    """SG3-T-256 layer geometries (up 2/4, down 2, 12/24 taps, the layer's crop padding), bias, clamp 256 hit.
    (An element of the upsampled plane within f32 rounding of the clamp edge takes the other side of the mask
    than in fp64 -- one such tie moves the relative error to ~5e-4 on a 556^2 plane -- hence 40^2 planes.)"""
    _, layers = sg3.layer_table(256)
    L = layers[li]
    g = torch.Generator().manual_seed(li)
    s = 40   # the geometry (up, down, taps, padding) is the layer's; a small plane keeps clamp-edge ties improbable
    x = torch.randn(2, 6, s, s, generator=g) * 30 + torch.linspace(-300, 300, 6).view(1, 6, 1, 1)
    b = torch.randn(6, generator=g)
    fu, fd = L["up_filter"], L["down_filter"]
    xd, bd = x.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    y = sg3_ops.filtered_lrelu(xd, fu.to(cuda), fd.to(cuda), bd, up=L["up"], down=L["down"], padding=L["padding"],
                               clamp=256)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.to(cuda))
    xr, br = x.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = sg3.filtered_lrelu(xr, fu.double(), fd.double(), br, up=L["up"], down=L["down"], padding=L["padding"],
                            clamp=256)
    u = sg3.upfirdn2d(xr.detach() + br.detach().view(1, -1, 1, 1), fu.double(), up=L["up"], padding=L["padding"],
                      gain=L["up"] ** 2)
    assert (u.abs() * np.sqrt(2) >= 256).any()   # the clamp mask takes part
    yr.backward(dy.double())
    assert _rel(xd.grad, xr.grad) < 1e-5 and _rel(bd.grad, br.grad) < 1e-5


@pytest.mark.parametrize("li", [0, 3, 8, 13, 14])
def test_synthesis_layer_gradients_fp32(cuda, gen256_frozen, li):
    """SynthesisLayer(x, w) with grad: d/dx and d/dw against autograd through the oracle layer in fp64.
    Tolerance 1e-3: the lrelu derivative jumps at 0, and upsampled elements within f32 rounding of 0 take the
    other slope than in fp64 -- measured 2e-5 .. 2e-4 relative, growing with the plane (148^2 x 512 x up 2)."""
    sd = _sd64(gen256_frozen)
    _, layers = sg3.layer_table(256)
    L = layers[li]
    g = torch.Generator().manual_seed(20 + li)
    x = torch.randn(2, L["in_channels"], L["in_size"], L["in_size"], generator=g)
    w = torch.randn(2, 512, generator=g)
    xd, wd = x.to(cuda).requires_grad_(True), w.to(cuda).requires_grad_(True)
    y = getattr(gen256_frozen.synthesis, L["name"])(xd, wd)
    r = torch.randn(y.shape, generator=g)
    (y * r.to(cuda)).sum().backward()
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = sg3.synthesis_layer(sd, L, xr, wr, dtype=torch.float64)
    assert (y.detach().cpu().double() - yr.detach()).abs().max().item() < 1e-4 * (1 + yr.abs().max().item())
    (yr * r.double()).sum().backward()
    ex, ew = _rel(xd.grad, xr.grad), _rel(wd.grad, wr.grad)
    print(f"[{L['name']}] rel grad error x {ex:.2e} w {ew:.2e}")
    assert ex < 1e-3 and ew < 1e-3


@pytest.mark.parametrize("li", [3, 8, 12, 13])
def test_synthesis_layer_gradients_bf16(cuda, gen256_frozen, li):
    """The bf16 training step of one SynthesisLayer (forward_train_nhwc in bf16, as the C5 / synthesis-gradient path
    runs it): d/dw, which reaches w only through the modulation scales (the oscale gradient is recovered as
    sum(dL/dy * (y - bias)) / oscale from the stored f16 output), and d/dx, against autograd through the
    fp64 oracle layer on the same bf16-rounded input.  Bound: 3x the error measured on MI355X (printed)."""
    sd = _sd64(gen256_frozen)
    _, layers = sg3.layer_table(256)
    L = layers[li]
    g = torch.Generator().manual_seed(40 + li)
    x = torch.randn(2, L["in_channels"], L["in_size"], L["in_size"], generator=g).to(torch.bfloat16).float()
    w = torch.randn(2, 512, generator=g)
    layer = getattr(gen256_frozen.synthesis, L["name"])
    xn = F.pad(x.permute(0, 2, 3, 1), (0, layer.cin_p - L["in_channels"])).to(cuda, torch.bfloat16)
    xd, wd = xn.requires_grad_(True), w.to(cuda).requires_grad_(True)
    y = layer.forward_train_nhwc(xd, wd, torch.bfloat16)[..., : L["out_channels"]].permute(0, 3, 1, 2)
    r = torch.randn(y.shape, generator=g)
    (y.float() * r.to(cuda)).sum().backward()
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = sg3.synthesis_layer(sd, L, xr, wr, dtype=torch.float64)
    (yr * r.double()).sum().backward()
    gx = xd.grad[..., : L["in_channels"]].permute(0, 3, 1, 2)
    ey = _rel(y, yr)
    ex, ew = _rel(gx, xr.grad), _rel(wd.grad, wr.grad)
    print(f"[{L['name']} bf16] rel error y {ey:.2e}, grad x {ex:.2e}, grad w {ew:.2e}")
    tx, tw = _BF16_LAYER_TOL[li]
    assert ex < tx and ew < tw


# (x, w) relative gradient error bounds of the bf16 layer test: ~3x the MI355X measurement (round 3: x / w
# 7.6e-3 / 7.4e-3 on L3, 9.8e-3 / 9.8e-3 on L8, 1.6e-2 / 1.5e-2 on L12, 1.7e-2 / 1.6e-2 on L13; forward 2.8e-3)
_BF16_LAYER_TOL = {3: (0.025, 0.025), 8: (0.03, 0.03), 12: (0.05, 0.05), 13: (0.05, 0.05)}


def test_synthesis_input_gradient(cuda, gen256_frozen):
    sd = _sd64(gen256_frozen)
    inp, _ = sg3.layer_table(256)
    w = torch.randn(3, 512, generator=torch.Generator().manual_seed(4))
    wd = w.to(cuda).requires_grad_(True)
    y = gen256_frozen.synthesis.input(wd)
    r = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
    (y * r.to(cuda)).sum().backward()
    wr = w.double().requires_grad_(True)
    yr = sg3.synthesis_input(sd, inp, wr, dtype=torch.float64)
    assert (y.detach().cpu().double() - yr.detach()).abs().max().item() < 1e-4 * (1 + yr.abs().max().item())
    (yr * r.double()).sum().backward()
    assert _rel(wd.grad, wr.grad) < 1e-4


def _oracle_synthesis_grad(ws):
    """dL/dws through the fp64 oracle synthesis: the committed fixture made by tests/golden/make_synthesis_grad.py
    (the same frozen generator, ws and r as below; ~4 CPU-minutes in fp64, so not recomputed on the GPU box)."""
    import os
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthesis_grad.npz"))
    assert np.array_equal(fx["ws"], ws.numpy())
    return torch.from_numpy(fx["dws"])


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 0.12), ("f16", 0.03)])
def test_synthesis_network_gradient_wrt_ws(cuda, gen256_frozen, precision, tol):
    """dL/dws through the whole frozen SG3-T-256 synthesis (input, 14 layers, ToRGB, output scale) against
    torch.autograd through the oracle in fp64 (committed fixture); the autograd forward equals the inference forward."""
    G = gen256_frozen
    ws = torch.randn(2, 16, 512, generator=torch.Generator().manual_seed(3)) * 0.7
    G.set_precision(precision)
    # f16: the f16 training path (synthesis.train_f16), the loss scaled by 2^12 as a GradScaler would
    scale = 4096.0 if precision == "f16" else 1.0
    G.synthesis.train_f16 = precision == "f16"
    try:
        with torch.no_grad():
            inf = G.synthesis(ws.to(cuda))
        wd = ws.to(cuda).requires_grad_(True)
        img = G.synthesis(wd)
        assert img.grad_fn is not None and img.shape == (2, 3, 256, 256)
        d_fwd = (img.detach() - inf).abs().max().item()
        r = torch.randn(img.shape, generator=torch.Generator().manual_seed(6))
        (img * r.to(cuda) * scale).sum().backward()
        wd.grad /= scale
    finally:
        G.set_precision("fp32")
        G.synthesis.train_f16 = False
    ref_grad = _oracle_synthesis_grad(ws)
    e = _rel(wd.grad, ref_grad)
    per_ws = [_rel(wd.grad[:, i], ref_grad[:, i]) for i in range(16)]
    print(f"[synthesis-{precision}] rel grad error {e:.2e}; per ws {[round(v, 5) for v in per_ws]}; "
          f"|train fwd - inference fwd| {d_fwd:.2e}")
    assert d_fwd < {"fp32": 1e-4, "bf16": 2e-2, "f16": 4e-3}[precision]
    assert e < tol


def test_synthesis_refuses_weight_gradients(cuda, gen256_frozen):
    G = gen256_frozen
    ws = torch.randn(1, 16, 512, device=cuda, requires_grad=True)
    G.synthesis.L3_52_512.weight.requires_grad_(True)
    try:
        out = G.synthesis(ws)            # the inference forward runs (grad-mode inference keeps working) ...
        with pytest.raises(nv.AutogradUnsupported):
            out.sum().backward()         # ... and the backward refuses: weight gradients are not implemented
    finally:
        G.synthesis.L3_52_512.weight.requires_grad_(False)


ENC64 = dict(img_resolution=64, img_channels=3, w_dim=512, num_ws=16, block_split=(5, 12), channel_base=1024,
             channel_max=64)


def test_compressor_training_loss_gradients(cuda, gen256_frozen):
    """The reference's training loss (rec MSE + kl_weight * KL to w_avg, ref :669-688; LPIPS excluded) through
    encoder -> frozen synthesis -> bilinear resize to the training resolution: every encoder gradient against the fp64
    oracle encoder (this call's eps and fc1) chained with dL/dws of the synthesis + resize + MSE.  That upstream
    gradient is the HIP fp32 path's on the oracle's latents: the fp64 CPU synthesis backward took ~30 s of the GPU
    suite, and the fp32 synthesis gradient is itself pinned to fp64 (test_synthesis_network_gradient_wrt_ws, committed
    fixture).  So this test checks the chaining: encoder forward, reparameterisation, KL, the autograd plumbing."""
    torch.manual_seed(0)
    enc = ic2.HVAE_VGG_Encoder(**ENC64).to(cuda)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1   # one image: the fp64 CPU synthesis backward dominates the test
    w_avg = torch.randn(1, 1, 512, generator=torch.Generator().manual_seed(10)) * 0.3
    xd = x.to(cuda)
    torch.manual_seed(1)
    wp, m, lv = enc(xd)
    img = gen256_frozen.synthesis(wp)
    img = ic2.resize_bilinear(img, (64, 64))
    loss = F.mse_loss(xd, img) + 0.01 * ict.kl_divergence(m, lv, w_avg.to(cuda))
    loss.backward()
    named = dict(enc.named_parameters())
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in named.items()}
    eps_all = ((wp - m) / torch.exp(0.5 * lv)).detach().cpu().double()
    eps = {"global": eps_all[:, :5], "medium": eps_all[:, 5:12], "fine": eps_all[:, 12:]}
    ow, om, olv = oe.encoder_forward(sd, x.double(), num_ws=16, block_split=(5, 12), w_dim=512,
                                     fine_fc1=(sd["fine_projector.fc1.weight"], sd["fine_projector.fc1.bias"]), eps=eps)
    # dL_rec/dws on the oracle's latents through the fp32 HIP synthesis + resize + MSE
    wo = ow.detach().float().to(cuda).requires_grad_(True)
    with torch.enable_grad():
        rec = F.mse_loss(xd, ic2.resize_bilinear(gen256_frozen.synthesis(wo), (64, 64)))
        rec.backward()
    oloss = rec.item() + 0.01 * ict.kl_divergence(om, olv, w_avg.double()).item()
    assert abs(loss.item() - oloss) < 1e-4 * abs(oloss)
    surrogate = (ow * wo.grad.double().cpu()).sum() + 0.01 * ict.kl_divergence(om, olv, w_avg.double())
    surrogate.backward()
    worst = {}
    gmax = max(sd[k].grad.norm().item() for k in named if sd[k].grad is not None)
    for k, p in named.items():
        if sd[k].grad is None:
            assert p.grad is None, k
            continue
        if sd[k].grad.norm().item() < 1e-8 * gmax:
            assert p.grad.norm().item() < 1e-4 * gmax, k
            continue
        worst[k] = _rel(p.grad, sd[k].grad)
    print(f"[compressor-train] max relative grad error {max(worst.values()):.2e} over {len(worst)} tensors")
    assert max(worst.values()) < 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:4]


@pytest.mark.parametrize("second_pass", [True, False])
def test_train_step_updates_encoder(cuda, gen256_frozen, second_pass):
    torch.manual_seed(0)
    enc = ic2.HVAE_VGG_Encoder(**ENC64).to(cuda)
    comp = ic2.StyleGAN3Compressor(enc, gen256_frozen, training_resolution=64)
    opt = ict.make_optimizer(enc, lr=1e-4)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    w_avg = gen256_frozen.mapping.w_avg.view(1, 1, -1)
    before = {k: v.detach().clone() for k, v in enc.named_parameters()}
    for _ in range(2):
        out = ict.train_step(comp, x, opt, w_avg, perceptual_weight=0.0, second_encoder_pass=second_pass)
    vals = {k: v.item() for k, v in out.items()}
    assert all(np.isfinite(v) for v in vals.values()), vals
    assert abs(vals["total_loss"] - (vals["rec_loss"] + 0.01 * vals["kl_loss"])) < 1e-5 * vals["total_loss"]
    changed = [k for k, v in enc.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(changed) >= len(before) // 2, changed
    assert all(p.grad is None for p in gen256_frozen.parameters())


def test_train_step_f16_loss_scaler(cuda, gen256_frozen):
    """BASELINE config 5's fp16 step (the reference's autocast + GradScaler, stylegan3_hvae_full.py:487,669,693-696):
    training.make_f16 + train_step(scaler=...).  The step's unscaled gradients agree with the fp32 step's on the same
    batch (f16 operands: a few 1e-2 relative in the worst tensor), the scale stays at 2^16 (no overflow on a clean
    step) and the parameters move; an injected overflow makes the scaler skip the step and halve its scale."""
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    w_avg = gen256_frozen.mapping.w_avg.view(1, 1, -1)
    grads = {}
    for prec in ("fp32", "bf16", "f16"):
        torch.manual_seed(0)
        enc = ic2.HVAE_VGG_Encoder(**ENC64).to(cuda)
        comp = ic2.StyleGAN3Compressor(enc, gen256_frozen, training_resolution=64)
        opt = ict.make_optimizer(enc, lr=1e-4)
        scaler = ict.make_f16(comp) if prec == "f16" else None
        if prec == "bf16":
            enc.set_precision("bf16")
            gen256_frozen.set_precision("bf16")
        before = {k: v.detach().clone() for k, v in enc.named_parameters()}
        try:
            torch.manual_seed(3)
            out = ict.train_step(comp, x, opt, w_avg, perceptual_weight=0.0, scaler=scaler)
        finally:
            gen256_frozen.set_precision("fp32")
            gen256_frozen.synthesis.train_f16 = False
        assert all(np.isfinite(v.item()) for v in out.values())
        # the optimizer's parameters hold unscaled gradients after the step (the scaler unscales them in place, or a
        # fused Adam, which takes the scale into its own kernel, writes them back unscaled); the fine projector's fc1,
        # re-created by every forward (ref :225-230), is not the optimizer's and keeps the scaled gradient
        held = {id(p) for grp in opt.param_groups for p in grp["params"]}
        grads[prec] = {k: v.grad.detach().clone() / (65536.0 if scaler is not None and id(v) not in held else 1.0)
                       for k, v in enc.named_parameters() if v.grad is not None}
        changed = [k for k, v in enc.named_parameters() if not torch.equal(v.detach(), before[k])]
        assert len(changed) >= len(before) // 2, changed
        if scaler is not None:
            assert scaler.get_scale() == 65536.0
            # an overflowed gradient: the step is skipped and the scale halved (the forward re-creates the fine
            # projector's fc1, ref :225-230, so the snapshot is taken after it)
            p0 = next(enc.parameters())
            opt.zero_grad()
            m = enc(x)[1]
            snap = {k: v.detach().clone() for k, v in enc.named_parameters()}
            loss = (m.float().sum() * 0 + p0.sum() * float("inf"))
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            assert scaler.get_scale() == 32768.0
            assert all(torch.equal(v.detach(), snap[k]) for k, v in enc.named_parameters())
    big = max(g.norm() for g in grads["fp32"].values())
    keys = [k for k in grads["fp32"] if grads["fp32"][k].norm() > 1e-6 * big]
    whole, top = {}, {}
    for prec in ("bf16", "f16"):
        rel = {k: _rel(grads[prec][k], grads["fp32"][k]) for k in keys}
        whole[prec] = _rel(torch.cat([grads[prec][k].flatten() for k in keys]),
                           torch.cat([grads["fp32"][k].flatten() for k in keys]))
        top[prec] = sorted(rel.items(), key=lambda kv: -kv[1])[:3]
        print(f"[train-step {prec} vs fp32] all gradients {whole[prec]:.2e}; worst tensors "
              + ", ".join(f"{k} {v:.2e}" for k, v in top[prec]))
    # two networks' backward on 16-bit operands: the errors compound through the encoder's GroupNorms (r4 measured
    # 9.9e-2 over the whole f16 gradient, 1.4e-1 in from_rgb); f16 (11-bit significands, loss-scaled) must do better
    # than the bf16 mode (8 bits), whose components are bounded against fp64 in the tests above
    assert whole["f16"] < whole["bf16"] and top["f16"][0][1] < 0.3


@pytest.mark.parametrize("li", [2, 5, 9, 12])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_flrelu_backward_kernel(cuda, gen256_frozen, li, mode):
    """ic2_flrelu_bwd_nhwc (fused: U recompute, adjoint down-FIR, lrelu'/clamp mask, adjoint up-FIR) on the
    SG3-T-256 layer geometries (up 2 and 4, the layers' crop / pad offsets) against autograd through the
    oracle's filtered_lrelu in fp64 on the same stored operands (bf16 mode: f16 input, bf16 output gradient).
    Clamp reached on a third of the channels."""
    L = gen256_frozen.synthesis.layers()[li]
    c, cp = L.out_channels, L.cout_p
    s = int(L.in_size[0]) + L.conv_kernel - 1
    g = torch.Generator().manual_seed(li)
    y = torch.randn(1, s, s, c, generator=g) * 3
    y[..., : c // 3] = y[..., : c // 3] * 60 + 150
    y = F.pad(y, (0, cp - c))
    dt = torch.float32 if mode == "fp32" else torch.bfloat16
    yd = y.to(cuda).requires_grad_(True)
    out = ao.FilteredLReluNHWC.apply(yd, L, dt)
    gout = F.pad(torch.randn(out.shape[:3] + (c,), generator=g), (0, cp - c)).to(dt)
    out.backward(gout.to(cuda))
    yr = (y if mode == "fp32" else y.half().float()).double()[..., :c].permute(0, 3, 1, 2).requires_grad_(True)
    _, layers = sg3.layer_table(256)
    Lr = layers[li]
    o = sg3.filtered_lrelu(yr, Lr["up_filter"].double(), Lr["down_filter"].double(), up=Lr["up"], down=Lr["down"],
                           padding=Lr["padding"], clamp=256)
    o.backward(gout.double()[..., :c].permute(0, 3, 1, 2))
    got = yd.grad.float().cpu()
    assert got.dtype == torch.float32 and (c == cp or got[..., c:].abs().max().item() == 0.0)
    e = _rel(got[..., :c].permute(0, 3, 1, 2), yr.grad)
    print(f"[flrelu-bwd L{li} {mode}] rel err {e:.2e}")
    assert e < 1e-3


@pytest.mark.parametrize("li", [2, 3, 5, 9, 10, 12])
@pytest.mark.parametrize("gscale,gdt", [(1.0, "bf16"), (1e-7, "bf16"), (1.0, "f16")])
def test_flrelu_backward_mfma_kernel(cuda, gen256_frozen, li, gscale, gdt):
    """The bf16 training path's FLR backward on MFMA (flrelu_bwd_mfma.hip: f16 x, bf16 gout, bf16 gx * oscale, the
    ydot partials of d oscale) on the SG3-T-256 layer geometries (up 2: L2, L9, L12; up 4: L3, L5, L10), against
    autograd through the oracle's filtered_lrelu in fp64 on the same stored operands.  Bound: the bf16 operands of
    its four gradient passes (2^-9 each) and the bf16 output; gscale 1e-7 puts dL/dout below the f16 range (the
    reason the gradient passes are bf16).  Clamp reached on a third of the channels; two samples, so the strip
    kernel's segments and several channel blocks are covered."""
    import ctypes
    L = gen256_frozen.synthesis.layers()[li]
    c, cp = L.out_channels, L.cout_p
    n = 1 if li == 10 else 2   # L10 (2 x 256 x 600^2 fp64 grids in the oracle) at one sample: test-time budget
    s = int(L.in_size[0]) + L.conv_kernel - 1
    so = int(L.out_size[0])
    g = torch.Generator().manual_seed(100 + li)
    y = torch.randn(n, s, s, c, generator=g) * 3
    y[..., : c // 3] = y[..., : c // 3] * 60 + 150
    y = F.pad(y, (0, cp - c)).half()
    tdt = torch.float16 if gdt == "f16" else torch.bfloat16
    gout = F.pad(torch.randn(n, so, so, c, generator=g) * gscale, (0, cp - c)).to(tdt)
    os_ = torch.rand(n, cp, generator=g) + 0.5
    bias = torch.randn(cp, generator=g)
    yd, gd_, osd, bd = y.to(cuda), gout.to(cuda), os_.to(cuda), bias.to(cuda)
    dc = torch.empty(n, s, s, cp, device=cuda, dtype=tdt)
    nyd = int(nv.query("ic2_flrelu_bwd_ydot_floats", n, cp, s, s, L.up_factor))
    ydot = torch.full([nyd], float("nan"), device=cuda)
    fu, fdn = L._fu, L._fd
    clamp = float(L.conv_clamp)
    rc = nv.load().ic2_flrelu_bwd_nhwc_ex(
        nv.ptr(yd), nv.F16, nv.ptr(gd_), nv.dtype_code(tdt), nv.ptr(dc), nv.dtype_code(tdt), n, cp, s, s, so, so,
        fu.ctypes.data_as(ctypes.c_void_p), fu.shape[0], fdn.ctypes.data_as(ctypes.c_void_p), fdn.shape[0],
        L.up_factor, L.down_factor, *L.padding, float(L.act_gain), 0.2, clamp, 0, nv.ptr(osd), nv.ptr(bd),
        nv.ptr(ydot), nyd, nv.stream_of(yd))
    assert rc == 0, nv.load().ic2_last_error().decode()
    torch.cuda.synchronize()
    yr = y.double()[..., :c].permute(0, 3, 1, 2).requires_grad_(True)
    _, layers = sg3.layer_table(256)
    Lr = layers[li]
    o = sg3.filtered_lrelu(yr, Lr["up_filter"].double(), Lr["down_filter"].double(), up=Lr["up"], down=Lr["down"],
                           padding=Lr["padding"], clamp=256)
    o.backward(gout.double()[..., :c].permute(0, 3, 1, 2))
    ref = yr.grad.permute(0, 2, 3, 1)  # dL/dy, NHWC
    got = dc.float().cpu()
    assert torch.isfinite(got).all() and (c == cp or got[..., c:].abs().max().item() == 0.0)
    e = _rel(got[..., :c], ref * os_.double()[:, None, None, :c])
    yd_ref = (ref * (y.double()[..., :c] - bias.double()[:c])).sum(dim=(1, 2))
    yd_got = ydot.view(n, -1, cp).sum(1).cpu()[:, :c]
    ey = _rel(yd_got, yd_ref)
    print(f"[flrelu-bwd-mfma L{li} {gdt} gscale {gscale:g}] rel err gx {e:.2e}, ydot {ey:.2e}")
    # the floor of both: U is recomputed in f16 (the forward's operands), so grid values within f16 rounding of 0 or
    # of the clamp take the other side of the lrelu / clamp than in fp64 (measured: bf16 gradients 5.7e-3 .. 7.7e-3,
    # f16 gradients 3.4e-3 .. 6.6e-3 -- the gradient operands' own rounding, 2^-9 vs 2^-12, is below it)
    assert e < 1.2e-2
    assert ey < 2e-2


@pytest.mark.parametrize("cp,hw,n", [(512, 38 * 38, 2), (192, 278 * 277, 1), (64, 1000, 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_scale_backward_kernel(cuda, cp, hw, n, dtype):
    """ic2_scale_bwd_nhwc: dx = da * xscale and d xscale = sum_p da * x (per-chunk partials summed on the host)."""
    g = torch.Generator().manual_seed(cp)
    da = torch.randn(n, hw, cp, generator=g).to(dtype)
    x = torch.randn(n, hw, cp, generator=g).to(dtype)
    xs = torch.randn(n, cp, generator=g)
    dad, xd, xsd = da.to(cuda), x.to(cuda), xs.to(cuda)
    dx = torch.empty_like(xd)
    npart = int(nv.query("ic2_scale_bwd_part_floats", n, hw, cp))
    part = torch.empty([npart], dtype=torch.float32, device=cuda)
    nv.call("ic2_scale_bwd_nhwc", nv.ptr(dad), nv.ptr(xd), nv.ptr(xsd), nv.ptr(dx), nv.dtype_code(dtype), n, hw, cp,
            nv.ptr(part), npart, nv.stream_of())
    ref_dx = (da.double() * xs.double()[:, None, :]).to(dtype)
    assert torch.equal(dx.cpu(), ref_dx) if dtype == torch.float32 else (dx.cpu().float() - ref_dx.float()).abs().max() \
        <= 2 ** -7 * ref_dx.float().abs().max()
    dxs = part.view(n, -1, cp).sum(1).cpu().double()
    ref = (da.double() * x.double()).sum(1)
    assert _rel(dxs, ref) < 1e-5


@pytest.mark.parametrize("cp,hw,n", [(512, 38 * 38, 2), (192, 278 * 277, 1), (96, 1000, 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_scale_forward_kernel(cuda, cp, hw, n, dtype):
    """ic2_scale_nhwc (the training path's a = x * xscale[n][c]): f32 exact, bf16 the product of the f32 scale and the
    bf16 input rounded once."""
    g = torch.Generator().manual_seed(cp + 1)
    x = torch.randn(n, hw, cp, generator=g).to(dtype)
    xs = torch.randn(n, cp, generator=g)
    xd, xsd = x.to(cuda), xs.to(cuda)
    a = torch.empty_like(xd)
    nv.call("ic2_scale_nhwc", nv.ptr(xd), nv.ptr(xsd), nv.ptr(a), nv.dtype_code(dtype), n, hw, cp, nv.stream_of())
    ref = (x.float() * xs[:, None, :]).to(dtype)  # one f32 product, rounded once (exact for f32)
    assert torch.equal(a.cpu(), ref)



def test_f16_train_step_graph_capture_replays_sane_losses(cuda):
    """the whole f16 training step (make_f16 + GradScaler, capturable fused Adam) captured in a
    graph and replayed twice gives finite rec_loss >= 0 that tracks the eager step (the reparameterisation noise
    differs between eager and replay, so within noise: 2x), and the weights move.  The round-4 negative replay loss
    (profiles/r4graph_c5_graph_ab.txt) does not reproduce on this tree (tools/graph_probe.py, profiles/
    r5_graph_probe.txt); the fine projector is fixed here (the reference's per-call fc1 draw goes through pinned host
    memory, which a capture refuses)."""
    import image_compression_2_amd as ic2
    from image_compression_2_amd import training as ict
    torch.manual_seed(0)
    enc = ic2.HVAE_VGG_Encoder(img_resolution=64, channel_base=1024, channel_max=64, fix_fine_projector=True).to(cuda)
    G = ic2.Generator(img_resolution=256).to(cuda).eval().requires_grad_(False)
    comp = ic2.StyleGAN3Compressor(enc, G, training_resolution=64)
    scaler = ict.make_f16(comp)
    opt = torch.optim.Adam(list(enc.parameters()), lr=1e-3, betas=(0.9, 0.999), fused=True, capturable=True)
    w_avg = G.mapping.w_avg.view(1, 1, -1)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(cuda)

    def step():
        return ict.train_step(comp, x, opt, w_avg, perceptual_weight=0.0, sync_gradients=1, scaler=scaler)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [float(step()["rec_loss"]) for _ in range(2)]
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    before = [p.detach().clone() for p in enc.parameters()]
    reps = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        reps.append((float(out["rec_loss"]), float(out["kl_loss"])))
    print(f"[graph f16] eager rec {eager}, replay (rec, kl) {reps}")
    ref = sum(eager) / len(eager)
    for rec, kl in reps:
        assert np.isfinite(rec) and np.isfinite(kl) and rec >= 0 and kl >= 0
        assert 0.5 * ref < rec < 2.0 * ref, (rec, eager)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, enc.parameters()))
    assert all(torch.isfinite(p).all() for p in enc.parameters())


def test_colsum_div_matches_torch_where_chain(cuda):
    """ic2_colsum_div (the d oscale / d xscale finish of the synthesis backward) equals the torch chain it replaced,
    where(den != 0, part.view(n, -1, c).sum(1) / den, 0), including zero denominators, and the plain column sum."""
    from image_compression_2_amd import _native as nv
    g = torch.Generator(device=cuda).manual_seed(0)
    for n, rows, c in ((3, 17, 96), (16, 256, 512), (1, 1, 32)):
        part = torch.randn(n, rows, c, device=cuda, generator=g)
        den = torch.randn(n, c, device=cuda, generator=g)
        den[:, ::7] = 0.0
        got = nv.colsum_div(part, n, c, den)
        s = part.double().sum(1)
        ref = torch.where(den != 0, s / torch.where(den != 0, den.double(), torch.ones_like(s)), torch.zeros_like(s))
        assert torch.allclose(got.double(), ref, rtol=1e-5, atol=1e-5 * float(ref.abs().max()))
        assert (got[:, ::7] == 0).all()
        assert torch.allclose(nv.colsum_div(part, n, c).double(), s, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("precision,gtol", [("fp32", 5e-5), ("f16", 2e-2)])
def test_train_step_shared_trunk_matches_two_encoder_passes(cuda, precision, gtol):
    """train_step's shared trunk (the reference's two encoder calls on one batch, :669 and :678, as one trunk and two
    projector heads) against two full encoder passes: the same losses (every value and RNG draw is the same) and the
    same gradients up to summation order."""
    import image_compression_2_amd as ic2
    from image_compression_2_amd import training as ict
    torch.manual_seed(0)
    enc = ic2.HVAE_VGG_Encoder(img_resolution=64, channel_base=1024, channel_max=64).to(cuda)
    torch.manual_seed(1)
    G = ic2.Generator(img_resolution=256).to(cuda).eval().requires_grad_(False)
    comp = ic2.StyleGAN3Compressor(enc, G, training_resolution=64)
    scaler = None
    if precision == "f16":
        scaler = ict.make_f16(comp)
    w_avg = G.mapping.w_avg.view(1, 1, -1)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(cuda)
    res = {}
    for shared in (True, False):
        opt = torch.optim.SGD(enc.parameters(), lr=0.0)   # no update: both runs see the same weights
        torch.manual_seed(11)
        out = ict.train_step(comp, x, opt, w_avg, perceptual_weight=0.0, sync_gradients=1, scaler=scaler,
                             shared_trunk=shared)
        res[shared] = ({k: float(v) for k, v in out.items()},
                       {k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None})
    (la, ga), (lb, gb) = res[True], res[False]
    print(f"[shared trunk {precision}] losses {la} vs {lb}")
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-6 * max(1.0, abs(lb[k])), (k, la[k], lb[k])
    assert ga.keys() == gb.keys()
    # a conv followed by a one-channel-per-group GroupNorm has an exactly zero bias gradient (sum of dy over the
    # group): both runs hold rounding noise there, bounded against the largest gradient instead
    gmax = max(float(g.norm()) for g in gb.values())
    errs = sorted(((_rel(ga[k], gb[k]) if float(gb[k].norm()) > 1e-6 * gmax
                    else float((ga[k] - gb[k]).norm()) / gmax, k) for k in gb), reverse=True)
    print(f"[shared trunk {precision}] worst gradients {[(k, round(e, 6)) for e, k in errs[:6]]}")
    assert errs[0][0] < gtol, errs[:6]


def test_scaled_layer_small_style_channels_f16(cuda, gen256_frozen):
    """the modulation-folded training layer (SynthLayerScaledNHWC) stores out = flrelu(y) * xs_next in
    f16 and recovers dL/dxs_next as sum(g * out) / xs_next, so a channel with |xs_next| in f16's subnormal range loses
    precision there.  Measured here on SG3-T-256 L8 with three channels at xs_next 1e-6 / 1e-5 / 1e-4 against the same
    layer in f32: every other channel's dL/dxs_next, and dL/da, stay at f16 level; the three small channels' own
    dL/dxs_next degrade (MI355X, round 5: 4.3e-2 / 5.1e-3 / 2.1e-3 relative at 1e-6 / 1e-5 / 1e-4, against 5.5e-4
    for the other channels and 3.9e-3 for dL/da; bounded at ~2.5x that).  The forward is the reference's fp16
    semantics (modulated_conv2d multiplies x by the styles in fp16 too), only this backward term is affected."""
    from image_compression_2_amd import autograd_ops as ao
    _, layers = sg3.layer_table(256)
    L = layers[8]
    layer = getattr(gen256_frozen.synthesis, L["name"])
    g = torch.Generator().manual_seed(8)
    n, s_in = 2, L["in_size"]
    a = torch.randn(n, s_in, s_in, layer.cin_p, generator=g) * 0.5
    a[..., L["in_channels"]:] = 0
    os_ = (torch.rand(n, layer.cout_p, generator=g) + 0.5) * 0.05
    xs = torch.rand(n, layer.cout_p, generator=g) + 0.5
    small = [3, 7, 11]
    for c, v in zip(small, (1e-6, 1e-5, 1e-4)):
        xs[:, c] = v
    res = {}
    for dt in (torch.float32, torch.float16):
        ad = a.to(cuda, dt).requires_grad_(True)
        xd = xs.to(cuda).requires_grad_(True)
        out = ao.SynthLayerScaledNHWC.apply(ad, os_.to(cuda), xd, layer, dt)
        r = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(cuda)
        (out.float() * r).sum().backward()
        res[dt] = (ad.grad.float().cpu(), xd.grad.float().cpu())
    (a32, x32), (a16, x16) = res[torch.float32], res[torch.float16]
    others = [c for c in range(L["out_channels"]) if c not in small]
    e_a = _rel(a16, a32)
    e_x = _rel(x16[:, others], x32[:, others])
    e_small = [_rel(x16[:, c], x32[:, c]) for c in small]
    print(f"[small styles f16] dL/da {e_a:.2e}, dL/dxs other channels {e_x:.2e}, small channels {e_small}")
    assert e_a < 2e-2 and e_x < 2e-2
    assert e_small[0] < 0.1 and e_small[1] < 1.5e-2 and e_small[2] < 6e-3
