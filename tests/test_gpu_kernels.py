"""GPU parity of every libic2ops kernel against the CPU oracle (op level)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from image_compression_2_amd import gumbel_softmax_compression as gsc
from image_compression_2_amd import metrics as icm
from image_compression_2_amd import sg3_ops
from image_compression_2_amd.stylegan3_hvae_full import _Act, _conv, _to_nhwc, _to_nchw
from oracle import encoder as oe
from oracle import metrics as om
from oracle import sg3

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _inference():
    """Inference tests run without a graph (grad mode works too: see test_gpu_path.py::test_grad_mode_inference)."""
    with torch.no_grad():
        yield


def _maxdiff(a, b):
    return (a.detach().float().cpu() - b.detach().float().cpu()).abs().max().item()


# ------------------------------------------------------------------ quantizers (bit-exact)
@pytest.mark.parametrize("bits", [4, 8, 10])
@pytest.mark.parametrize("tag", ["rand", "adv"])
def test_quantize_uniform_bit_exact(cuda, golden_dir, bits, tag):
    d = np.load(os.path.join(golden_dir, "quantizers.npz"))
    w = torch.from_numpy(d[f"uniform_b{bits}_{tag}_w"]).to(cuda)
    q, idx = ic2.quantize_uniform(w, bits, return_indices=True)
    assert torch.equal(q.cpu(), torch.from_numpy(d[f"uniform_b{bits}_{tag}_q"]))
    assert torch.equal(idx.cpu().long(), oe.uniform_indices(w.cpu(), bits))


@pytest.mark.parametrize("n", [1, 3, 5, 4097])
def test_quantize_uniform_ragged_sizes(cuda, n):
    w = (torch.rand(n, generator=torch.Generator().manual_seed(n)) * 3 - 1.5)
    q = ic2.quantize_uniform(w.to(cuda), 8)
    assert torch.equal(q.cpu(), oe.quantize_uniform(w, 8))


def test_codebook_argmin_bit_exact(cuda, golden_dir):
    d = np.load(os.path.join(golden_dir, "quantizers.npz"))
    z = torch.from_numpy(d["codebook_z"]).to(cuda)
    cb = torch.from_numpy(d["codebook"]).to(cuda)
    idx, hist = gsc.codebook_argmin(z, cb, hist=True)
    ref = d["codebook_idx"]
    assert np.array_equal(idx.cpu().numpy(), ref)
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), np.bincount(ref, minlength=256))


def test_codebook_lookup_and_oob(cuda):
    cb = oe.codebook().to(cuda)
    codes = torch.randint(0, 256, (2, 16, 512), generator=torch.Generator().manual_seed(0))
    w, flag = gsc.codebook_lookup(codes.to(cuda), cb)
    assert torch.equal(w.cpu(), oe.codebook_lookup(codes))
    assert flag.item() == 0
    codes[0, 0, 0] = 300
    _, flag = gsc.codebook_lookup(codes.to(cuda), cb)
    assert flag.item() == 1
    with pytest.raises(IndexError):
        gsc.check_codes(flag, 256)
    codes[0, 0, 0] = -1
    _, flag = gsc.codebook_lookup(codes.to(cuda), cb)
    assert flag.item() == 1


@pytest.mark.parametrize("hard", [False, True])
def test_gumbel_softmax_with_given_noise(cuda, hard):
    g = torch.Generator().manual_seed(3)
    z = torch.rand(2, 4, 64, generator=g) * 2.2 - 1.1
    noise = -torch.empty(z.numel(), 256).exponential_(generator=g).log()
    disc_mod = ic2.GumbelSoftmaxDiscretization(64, 256, temperature=0.7).to(cuda)
    disc, perp, idx = disc_mod(z.to(cuda), hard=hard, gumbel_noise=noise.to(cuda))
    rdisc, rperp, ridx = oe.gumbel_forward(z, noise, torch.exp(torch.ones(1) * np.log(0.7)), hard)
    assert torch.equal(idx.cpu(), ridx)
    assert _maxdiff(disc, rdisc) < 1e-5
    assert abs(perp.item() - rperp.item()) < 1e-3 * rperp.item()


@pytest.mark.parametrize("case", range(4))
def test_gumbel_forward_matches_reference_golden(cuda, golden_dir, case):
    """The fused Gumbel kernel fed the noise the REFERENCE drew (replayed from its seed; the hash pins the
    replay) against the reference's own outputs (tests/golden/gumbel_forward.npz, made by make_golden.py
    from gumbel_softmax_compression.py:73-129): soft / hard, learnable / fixed temperature, tau != 1."""
    import hashlib
    d = np.load(os.path.join(golden_dir, "gumbel_forward.npz"))
    learn, tau, hard, seed = d[f"c{case}_meta"]
    z = torch.from_numpy(d["z"])
    noise = torch.from_numpy(d["noise"])  # what the reference drew (replay check: test_gumbel_noise_replay)
    assert hashlib.sha256(noise.numpy().tobytes()).digest() == d[f"c{case}_noise_sha256"].tobytes()
    mod = ic2.GumbelSoftmaxDiscretization(z.shape[-1], 256, temperature=float(tau), learnable_temp=bool(learn))
    mod = mod.to(cuda).eval()
    with torch.no_grad():
        disc, perp, idx = mod(z.to(cuda), hard=bool(hard), gumbel_noise=noise.to(cuda))
    assert torch.equal(idx.cpu(), torch.from_numpy(d[f"c{case}_idx"]))
    assert _maxdiff(disc, torch.from_numpy(d[f"c{case}_disc"])) < 2e-6
    rp = float(d[f"c{case}_perplexity"])
    assert abs(perp.item() - rp) < 1e-4 * rp


def test_gumbel_softmax_generated_noise_statistics(cuda):
    torch.manual_seed(0)
    z = (torch.rand(4, 16, 512) * 2 - 1).to(cuda)
    mod = ic2.GumbelSoftmaxDiscretization(512, 256).to(cuda).eval()
    disc, perp, idx = mod(z, hard=True)
    cb = mod.codebook
    # hard straight-through output is a codebook value up to one rounding
    nearest = cb[torch.argmin((disc.reshape(-1, 1) - cb.reshape(1, -1)).abs(), 1)]
    assert (disc.reshape(-1) - nearest).abs().max().item() < 1e-6
    # gumbel noise dominates the 2/255 logit gaps: most codes differ from argmin
    frac_same = (nearest == cb[idx]).float().mean().item()
    assert frac_same < 0.2
    assert 100 < perp.item() <= 256


# ------------------------------------------------------------------ SG3 ops vs oracle
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.bfloat16, 2e-2)])
def test_bias_act(cuda, dtype, tol):
    x = torch.randn(2, 5, 7, 9)
    b = torch.randn(5)
    for act, kw in (("linear", {}), ("lrelu", dict(alpha=0.1, gain=1.7, clamp=1.5))):
        y = sg3_ops.bias_act(x.to(cuda, dtype), b.to(cuda), act=act, **kw)
        r = sg3.bias_act(x.to(dtype).float(), b, act=act, **kw)
        assert _maxdiff(y, r) <= tol * (1 + r.abs().max().item())


UFD_CASES = [
    dict(up=2, down=1, padding=[5, 6, 5, 6], taps=12, flip=False),
    dict(up=1, down=2, padding=0, taps=12, flip=False),
    dict(up=4, down=2, padding=[-6, -9, -6, -9], taps=24, flip=True),
    dict(up=2, down=2, padding=[1, 0, 2, 3], taps=5, flip=False),
]


@pytest.mark.parametrize("case", range(len(UFD_CASES)))
@pytest.mark.parametrize("ndim", [1, 2])
def test_upfirdn2d(cuda, case, ndim):
    c = UFD_CASES[case]
    g = torch.Generator().manual_seed(case)
    x = torch.randn(2, 3, 20, 17, generator=g)
    f = torch.rand(c["taps"], generator=g)
    if ndim == 2:
        f = torch.outer(f, torch.rand(c["taps"], generator=g))
    kw = dict(up=c["up"], down=c["down"], padding=c["padding"], flip_filter=c["flip"], gain=c["up"] ** 2)
    y = sg3_ops.upfirdn2d(x.to(cuda), f.to(cuda), **kw)
    r = sg3.upfirdn2d(x, f, **kw)
    assert y.shape == r.shape
    assert _maxdiff(y, r) < 1e-4 * (1 + r.abs().max().item())


FLR_CASES = [  # (up, down, taps_u, taps_d, padding, in size)
    (2, 2, 12, 12, [9, 8, 9, 8], 38),
    (4, 2, 24, 12, [-6, -9, -6, -9], 38),
    (2, 2, 12, 12, [-11, -12, -11, -12], 40),
    (1, 2, 1, 12, [3, 2, 3, 2], 21),   # no fused instance -> HIP composition
]


@pytest.mark.parametrize("case", range(len(FLR_CASES)))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_filtered_lrelu_nchw(cuda, case, dtype):
    up, down, tu, td, pad, s = FLR_CASES[case]
    g = torch.Generator().manual_seed(10 + case)
    x = torch.randn(2, 19, s, s, generator=g) * 3
    b = torch.randn(19, generator=g)
    fu = sg3.design_lowpass_filter(tu, 8.0, 4.0, 64) if tu > 1 else None
    fd = sg3.design_lowpass_filter(td, 8.0, 4.0, 64) if td > 1 else None
    kw = dict(up=up, down=down, padding=pad, gain=np.sqrt(2), slope=0.2, clamp=5.0)
    y = sg3_ops.filtered_lrelu(x.to(cuda, dtype), None if fu is None else fu.to(cuda),
                               None if fd is None else fd.to(cuda), b.to(cuda), **kw)
    r = sg3.filtered_lrelu(x.to(dtype).double(), None if fu is None else fu.double(),
                           None if fd is None else fd.double(), b.double(), **kw)
    assert y.shape == r.shape and y.dtype == dtype
    tol = 2e-5 if dtype == torch.float32 else 3e-2
    assert _maxdiff(y, r) < tol * (1 + r.abs().max().item())


@pytest.mark.parametrize("case", range(3))
def test_flrelu_nhwc_bf16_bias(cuda, case):
    """ic2_flrelu_nhwc with bf16 input, bf16 output and a bias.  The bias keeps the call off the MFMA kernels, so it
    runs the VALU kernel on the bf16 NHWC tile (16x16), which no other test reaches: up 2 / up 4, positive and
    negative padding, outputs that are no multiple of the tile.  Against the fp64 reference composition on the
    bf16-rounded input, at test_filtered_lrelu_nchw's bf16 bar (same kernel template); the NaN pre-fill shows every
    output element is written."""
    import ctypes
    up, down, tu, td, pad, s = FLR_CASES[case]
    n, c_p = 2, 32
    g = torch.Generator().manual_seed(30 + case)
    x = (torch.randn(n, c_p, s, s, generator=g) * 3).bfloat16()
    b = torch.randn(c_p, generator=g)
    fu = sg3.design_lowpass_filter(tu, 8.0, 4.0, 64)
    fd = sg3.design_lowpass_filter(td, 8.0, 4.0, 64)
    so = (s * up + pad[0] + pad[1] - (tu - 1) - (td - 1) + (down - 1)) // down
    xd = x.permute(0, 2, 3, 1).contiguous().to(cuda)
    bd = b.to(cuda)
    out = torch.full((n, so, so, c_p), float("nan"), device=cuda, dtype=torch.bfloat16)
    fun, fdn = fu.float().contiguous().numpy(), fd.float().contiguous().numpy()
    nv.call("ic2_flrelu_nhwc", nv.ptr(xd), nv.ptr(out), nv.BF16, nv.BF16, n, c_p, s, s, so, so,
            fun.ctypes.data_as(ctypes.c_void_p), tu, fdn.ctypes.data_as(ctypes.c_void_p), td, nv.ptr(bd), up, down, *pad,
            float(np.sqrt(2)), 0.2, 5.0, 0, None, nv.stream_of(xd))
    torch.cuda.synchronize()
    r = sg3.filtered_lrelu(x.double(), fu.double(), fd.double(), b.double(), up=up, down=down, padding=pad,
                           gain=np.sqrt(2), slope=0.2, clamp=5.0)
    y = out.float().cpu().permute(0, 3, 1, 2)
    assert y.shape == r.shape
    assert torch.isfinite(y).all()
    d = _maxdiff(y, r)
    print(f"max|diff| {d:.3e}  max|ref| {r.abs().max().item():.3e}")
    assert d < 3e-2 * (1 + r.abs().max().item())


# ------------------------------------------------------------------ fused FLR, synthesis (NHWC) path
@pytest.fixture(scope="module")
def gen256_bf16_layers():
    torch.manual_seed(1)
    return ic2.Generator(img_resolution=256).synthesis.layers()


@pytest.mark.parametrize("layer", [0, 3, 5, 10, 13])
@pytest.mark.parametrize("c_p", [32, 64])
@pytest.mark.parametrize("in_dtype,out_dtype", [(torch.bfloat16, torch.bfloat16), (torch.float16, torch.bfloat16),
                                                (torch.float16, torch.float16)])
def test_flrelu_nhwc_bf16_matches_oracle(cuda, gen256_bf16_layers, layer, c_p, in_dtype, out_dtype):
    """The NHWC filtered-lrelu with bf16 or f16 output (MFMA formulation, f16 operands) on SG3-T-256 layer
    geometries (up 2 / up 4, positive and negative padding), bf16 or f16 input, with a post_scale,
    against the fp64 reference composition."""
    import ctypes
    L = gen256_bf16_layers[layer]
    n = 2
    conv = int(L.in_size[0]) + 2
    s_out = int(L.out_size[0])
    g = torch.Generator().manual_seed(20 + layer)
    x = (torch.randn(n, c_p, conv, conv, generator=g) * 2).to(in_dtype).float()
    x[:, :, :3, :5] = 300.0  # exercises the clamp
    ps = torch.rand(n, c_p, generator=g) + 0.5
    xd = x.permute(0, 2, 3, 1).contiguous().to(cuda, in_dtype)
    out = torch.empty(n, s_out, s_out, c_p, device=cuda, dtype=out_dtype)
    psd = ps.to(cuda)
    nv.call("ic2_flrelu_nhwc", nv.ptr(xd), nv.ptr(out), nv.dtype_code(in_dtype), nv.dtype_code(out_dtype), n, c_p,
            conv, conv, s_out,
            s_out, L._fu.ctypes.data_as(ctypes.c_void_p), L._fu.shape[0], L._fd.ctypes.data_as(ctypes.c_void_p),
            L._fd.shape[0], None, L.up_factor, L.down_factor, *L.padding, float(np.sqrt(2)), 0.2, 256.0, 0,
            nv.ptr(psd), nv.stream_of(xd))
    torch.cuda.synchronize()
    r = sg3.filtered_lrelu(x.double(), torch.from_numpy(L._fu).double(), torch.from_numpy(L._fd).double(), None,
                           up=L.up_factor, down=L.down_factor, padding=L.padding, gain=np.sqrt(2), slope=0.2,
                           clamp=256.0) * ps.double()[:, :, None, None]
    y = out.float().cpu().permute(0, 3, 1, 2)
    assert y.shape == r.shape
    err = (y.double() - r).abs()
    scale = r.abs().max().item()
    assert err.max().item() < 2e-2 * (1 + scale), (err.max().item(), scale)
    assert err.mean().item() < 2e-3 * (1 + r.abs().mean().item())
    if out_dtype == torch.float16:
        # the f16 FIR operands (taps and intermediates, 2^-11) bound the error, not the output rounding
        assert err.max().item() < 4e-3 * (1 + scale), (err.max().item(), scale)


@pytest.mark.parametrize("layer", [0, 2, 6, 8, 10, 13])
@pytest.mark.parametrize("c_p", [32, 64])
def test_flrelu_nhwc16_equals_nhwc(cuda, gen256_bf16_layers, layer, c_p):
    """The channel-blocked hand-off (ic2_flrelu_nhwc16 on [n][c_p/16][h][w][16]) only changes the addressing of
    the fused kernel's input tiles: its output is bit-identical to ic2_flrelu_nhwc on the same values in NHWC
    (narrow and wide tiles, up 2 and up 4, both paddings), post_scale included."""
    import ctypes
    L = gen256_bf16_layers[layer]
    n = 2
    conv = int(L.in_size[0]) + 2
    s_out = int(L.out_size[0])
    g = torch.Generator().manual_seed(60 + layer)
    x = (torch.randn(n, conv, conv, c_p, generator=g) * 2).to(torch.float16)
    x[:, :4, :6, :] = 300.0
    ps = (torch.rand(n, c_p, generator=g) + 0.5).to(cuda)
    xd = x.to(cuda)
    xb = x.reshape(n, conv, conv, c_p // 16, 16).permute(0, 3, 1, 2, 4).contiguous().to(cuda)
    outs = []
    for fn, src in (("ic2_flrelu_nhwc", xd), ("ic2_flrelu_nhwc16", xb)):
        out = torch.full((n, s_out, s_out, c_p), float("nan"), device=cuda, dtype=torch.bfloat16)
        nv.call(fn, nv.ptr(src), nv.ptr(out), nv.F16, nv.BF16, n, c_p, conv, conv, s_out, s_out,
                L._fu.ctypes.data_as(ctypes.c_void_p), L._fu.shape[0], L._fd.ctypes.data_as(ctypes.c_void_p),
                L._fd.shape[0], None, L.up_factor, L.down_factor, *L.padding, float(np.sqrt(2)), 0.2, 256.0, 0,
                nv.ptr(ps), nv.stream_of(src))
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("cin,cout,size,n", [(512, 512, 12, 2), (512, 362, 20, 2), (256, 192, 40, 2),
                                             (192, 128, 66, 2), (128, 128, 70, 1), (96, 64, 48, 2), (32, 64, 40, 2)])
def test_conv_nhwc16_equals_nhwc(cuda, cin, cout, size, n):
    """ic2_conv_igemm with out_layout NHWC16 (f16, the synthesis conv -> filtered-lrelu hand-off) stores exactly the
    values of the NHWC output, channel-blocked, for whichever kernel the launch plan picks (8-phase GEMM, halo
    GEMM, halo conv, plain / split-K implicit GEMM); padded output channels included."""
    cin_p, cout_p = nv.pad_synth(cin), nv.pad_synth(cout)
    g = torch.Generator().manual_seed(cin + cout + size)
    x = torch.zeros(n, size, size, cin_p)
    x[..., :cin] = torch.randn(n, size, size, cin, generator=g)
    w = torch.zeros(cout_p, 3, 3, cin_p)
    w[:cout, :, :, :cin] = torch.randn(cout, 3, 3, cin, generator=g) / np.sqrt(9 * cin)
    osc = (torch.rand(n, cout_p, generator=g) + 0.5).to(cuda)
    bias = torch.randn(cout_p, generator=g).to(cuda)
    xd, wd = x.to(cuda, torch.bfloat16), w.to(cuda, torch.bfloat16)
    ho = size
    ys = {}
    for lay in (nv.NHWC, nv.NHWC16):
        y = torch.full((n * ho * ho * cout_p,), float("nan"), device=cuda, dtype=torch.float16)
        nv.conv_igemm(nv.ptr(xd), nv.ptr(wd), nv.ptr(y), nv.BF16, nv.F16, n, size, size, cin_p, cout_p, cout, 3, 3, 1,
                      ho, ho, nv.ptr(osc), nv.ptr(bias), 0, 0.0, 1.0, -1.0, 1.0, lay, nv.stream_of(xd), cuda)
        ys[lay] = y
    torch.cuda.synchronize()
    a = ys[nv.NHWC].view(n, ho, ho, cout_p)
    b = ys[nv.NHWC16].view(n, cout_p // 16, ho, ho, 16).permute(0, 2, 3, 1, 4).reshape(n, ho, ho, cout_p)
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a, b)


def test_f16_saturation_semantics(cuda, gen256_bf16_layers):
    """bf16 mode hands the filtered lrelu the modulated-conv output as f16 (its MFMA operand type), so a
    pre-activation beyond +-65504 saturates BEFORE the up-FIR, while the reference's fp32 CPU path clamps (at
    conv_clamp 256) only AFTER it; SG3's own CUDA path has the same f16 range in its fp16 layers.  Pinned:
    (1) the conv epilogue saturates to exactly +-65504 (no inf / NaN reaches the FIR); (2) the filtered lrelu of
    the saturated tensor equals the oracle on that tensor; (3) against the unsaturated oracle the outputs differ
    only inside the FIR support of a saturated pixel (DESIGN.md (c) records the measured deviation)."""
    import ctypes
    # (1) conv epilogue, f16 output
    g = torch.Generator().manual_seed(90)
    x = torch.randn(1, 8, 8, 32, generator=g).to(torch.bfloat16)
    x[0, 3, 3, :] = 3000.0
    w = (torch.randn(32, 1, 1, 32, generator=g) * 8).to(torch.bfloat16)
    y = torch.empty(1, 8, 8, 32, device=cuda, dtype=torch.float16)
    xd, wd = x.to(cuda), w.to(cuda)
    nv.conv_igemm(nv.ptr(xd), nv.ptr(wd), nv.ptr(y), nv.BF16, nv.F16, 1, 8, 8, 32, 32, 32, 1, 1, 0, 8, 8, None, None,
                  0, 0.0, 1.0, -1.0, 1.0, nv.NHWC, nv.stream_of(xd), cuda)
    torch.cuda.synchronize()
    ref = torch.einsum("nhwc,oc->nhwo", x.double(), w.double()[:, 0, 0])
    assert torch.isfinite(y).all() and (ref.abs() > 65504).any()
    assert torch.equal(y.cpu().double()[ref.abs() > 65520], ref.clamp(-65504, 65504)[ref.abs() > 65520])
    # (2) + (3) filtered lrelu of a tensor with saturated pixels (SG3-T-256 L8 geometry)
    L = gen256_bf16_layers[8]
    n, c_p, conv, s_out = 1, 32, int(L.in_size[0]) + 2, int(L.out_size[0])
    xr = torch.randn(n, c_p, conv, conv, generator=g) * 2
    hot = [(20, 30), (75, 75), (140, 9)]
    for (py, px) in hot:
        xr[:, :, py, px] = 2.0e5 * torch.sign(torch.randn(c_p, generator=g))[None, :]
    xs = xr.clamp(-65504, 65504).to(torch.float16).float()
    xd = xs.permute(0, 2, 3, 1).contiguous().to(cuda, torch.float16)
    out = torch.empty(n, s_out, s_out, c_p, device=cuda, dtype=torch.bfloat16)
    nv.call("ic2_flrelu_nhwc", nv.ptr(xd), nv.ptr(out), nv.F16, nv.BF16, n, c_p, conv, conv, s_out, s_out,
            L._fu.ctypes.data_as(ctypes.c_void_p), L._fu.shape[0], L._fd.ctypes.data_as(ctypes.c_void_p),
            L._fd.shape[0], None, L.up_factor, L.down_factor, *L.padding, float(np.sqrt(2)), 0.2, 256.0, 0, None,
            nv.stream_of(xd))
    torch.cuda.synchronize()
    kw = dict(up=L.up_factor, down=L.down_factor, padding=L.padding, gain=np.sqrt(2), slope=0.2, clamp=256.0)
    fu, fd = torch.from_numpy(L._fu).double(), torch.from_numpy(L._fd).double()
    r_sat = sg3.filtered_lrelu(xs.double(), fu, fd, None, **kw)
    yv = out.float().cpu().permute(0, 3, 1, 2).double()
    assert (yv - r_sat).abs().max().item() < 2e-2 * (1 + r_sat.abs().max().item())
    # the saturation alone (f32 elsewhere) against the unsaturated reference
    r_raw = sg3.filtered_lrelu(xr.double(), fu, fd, None, **kw)
    r_clp = sg3.filtered_lrelu(xr.clamp(-65504, 65504).double(), fu, fd, None, **kw)
    # outputs whose input support holds no saturated pixel are unaffected by the saturation
    near = torch.zeros(s_out, s_out, dtype=torch.bool)
    rad = (L.up_taps // L.up_factor + L.down_taps) // 2 + 2
    for (py, px) in hot:
        cy, cx = (py * L.up_factor + L.padding[2]) // L.down_factor, (px * L.up_factor + L.padding[0]) // L.down_factor
        near[max(cy - rad, 0):cy + rad + 1, max(cx - rad, 0):cx + rad + 1] = True
    dev = (r_raw - r_clp).abs()
    assert dev[..., ~near].max().item() == 0.0
    print(f"[f16-saturation] max |raw - saturated| inside the support of 3 saturated pixels: "
          f"{dev[..., near].max().item():.3f} (outputs clamp at 256)")


# ------------------------------------------------------------------ implicit-GEMM conv (MFMA)
IGEMM_CASES = [(3, 32, 19, 1, 0), (64, 96, 12, 1, 0), (181, 128, 9, 2, 0), (512, 512, 6, 2, 0),
               (256, 362, 10, 2, 1), (96, 64, 13, 1, 2), (128, 181, 11, 2, 3), (512, 256, 7, 2, 4),
               (181, 192, 9, 2, 5), (512, 512, 6, 2, 6), (181, 256, 9, 1, 6), (128, 512, 21, 1, 6),
               (64, 300, 10, 1, 6), (128, 128, 21, 1, 7), (64, 96, 13, 1, 7), (192, 64, 17, 0, 7),
               (64, 362, 10, 1, 7)]


def _child_conv_cases(env, cases, dtype, n=None):
    """_conv_case over `cases` in ONE child process with the knob environment `env` (the knobs are read once per
    process); the child tries every case and reports all that fail."""
    import subprocess, sys
    code = (f"import sys, torch; sys.path.insert(0, {repr(str(os.getcwd()))});"
            f"from tests.test_gpu_kernels import _conv_cases_report; _conv_cases_report({cases!r}, {dtype}, {n!r})")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, IC2_DEV="1", **env), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]


def _conv_cases_report(cases, dtype, n=None):
    bad = []
    for c in cases:
        try:
            _conv_case(*c, dtype=dtype, **({"n": n} if n else {}))
        except AssertionError as e:
            bad.append((c, str(e)[:300]))
    assert not bad, f"failing cases: {bad}"


@pytest.mark.parametrize("cin,cout,size,pad,tile", [c for c in IGEMM_CASES if c[4] == 0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_conv_igemm(cuda, cin, cout, size, pad, tile, dtype):
    """The default plan's implicit-GEMM instances against F.conv2d in fp64."""
    _conv_case(cin, cout, size, pad, dtype)


@pytest.mark.parametrize("tile", sorted({c[4] for c in IGEMM_CASES} - {0}))
@pytest.mark.parametrize("dtype", [torch.float32, "torch.bfloat16", "torch.float16"])
def test_conv_igemm_forced_tiles(cuda, tile, dtype):
    """Every bf16 / f16 tile instance, forced by the knob IC2_IGEMM_TILE (IC2_DEV=1; read once per process, so each
    tile's cases run in one child process), against F.conv2d in fp64; fp32 has one tile and runs in-process."""
    cases = [c[:4] for c in IGEMM_CASES if c[4] == tile]
    if dtype == torch.float32:
        for c in cases:
            _conv_case(*c, dtype)
        return
    _child_conv_cases({"IC2_IGEMM_TILE": str(tile)}, cases, dtype)


@pytest.mark.parametrize("cin,cout,size,pad", [(32, 32, 150, 1), (3, 32, 160, 1), (32, 64, 151, 2), (64, 32, 149, 2),
                                              (64, 64, 149, 1), (60, 50, 150, 0), (81, 51, 150, 2), (96, 32, 149, 1)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv_halo_kernel(cuda, cin, cout, size, pad, dtype):
    """The halo direct conv (bf16 / f16 3x3, cin_p / cout_p in {32, 64}, >= 64K output pixels: encoder block 0,
    SG3-T-1024 L12/L13) against F.conv2d in fp64, with ragged 8 x 32 tiles at the right / bottom edges."""
    assert 3 * (size + 2 * pad - 2) ** 2 >= 65536
    _conv_case(cin, cout, size, pad, dtype)


HG4_CASES = [(64, 128, 45, 2), (96, 128, 40, 1), (128, 181, 40, 2), (192, 192, 33, 1), (256, 256, 30, 2),
             (32, 256, 29, 1), (128, 384, 20, 1), (64, 320, 21, 1), (181, 128, 37, 2), (81, 51, 37, 2), (64, 64, 33, 1),
             (384, 128, 24, 1), (512, 192, 21, 1)]


@pytest.mark.parametrize("dtype", ["torch.bfloat16", "torch.float16"])
def test_conv_halo_gemm4(cuda, dtype):
    """The 4-wave halo implicit GEMM (hg4: 32-channel blocks, two workgroups per CU) forced on every instance
    (knob IC2_HG4=2 under IC2_DEV=1, read once per process, so in a child process): 64 / 96 / 128 / 192 output channels
    per workgroup, 8 x 32 / 16 x 16 / 4 x 32 / 8 x 16 pixel tiles, cin_p a multiple of 32 but not of 64 (96, 192 -> 192),
    partial o-tiles (320 = 2.5 x 128), ragged tile edges, pad 1 and 2 -- against F.conv2d in fp64."""
    _child_conv_cases({"IC2_HG4": "2"}, HG4_CASES, dtype, n=4)


@pytest.mark.parametrize("dtype", ["torch.bfloat16", "torch.float16"])
def test_conv_halo_gemm4_o192_outputs(cuda, dtype):
    """192-wide outputs on both hg4 forms, hg4 forced with IC2_HG4=2 in a child process: two 96-wide o-tiles on 32-wide
    pixel tiles (waves 2-3 issue one weight DMA fewer per tap) or one 192-wide o-tile on 16-wide ones, whichever pads
    the output less, against F.conv2d in fp64: 181 -> 192 padded outputs, ragged tiles.  The plan query, asked in a
    child under the same environment, must say that the cases still cover both forms."""
    import subprocess, sys
    cases = [(128, 181, 40, 2), (256, 192, 31, 2), (64, 192, 30, 1)]
    dt = {"torch.bfloat16": nv.BF16, "torch.float16": nv.F16}[dtype]
    code = (f"import sys; sys.path.insert(0, {repr(str(os.getcwd()))}); from image_compression_2_amd import _native as nv\n"
            f"for cin, cout, size, pad in {cases!r}:\n"
            f"    print(nv.conv_plan({dt}, {dt}, nv.NHWC, 4, size, size, nv.pad32(cin), nv.pad32(cout), cout, 3, 3, pad))")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, IC2_DEV="1", IC2_HG4="2"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    f16 = "_f16" if dt == nv.F16 else ""
    assert r.stdout.split() == ["hg4_o192_w16_s4" + f16, "hg4_o192_w16_s4" + f16, "hg4_o96_w32_p2" + f16], r.stdout
    _child_conv_cases({"IC2_HG4": "2"}, cases, dtype, n=4)


@pytest.mark.parametrize("cin,cout,size,pad,n", [(512, 512, 12, 1, 3), (1024, 320, 9, 1, 2), (768, 256, 7, 2, 5),
                                                 (512, 512, 2, 1, 8)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv_g8_splitk(cuda, cin, cout, size, pad, n, dtype):
    """Small grids of the 8-phase 256 x 256 kernel split K over gridDim.y (slices of >= 8 K-tiles, zero tiles past a
    slice's end, the split-K combine): the plan picks it on these shapes (partial o-tiles: 320; 2 x 2 images) and
    the result matches F.conv2d in fp64."""
    ho = size + 2 * pad - 2
    dc = nv.F16 if dtype == torch.float16 else nv.BF16
    assert nv.conv_plan(dc, dc, nv.NHWC, n, size, size, cin, nv.pad32(cout), cout, 3, 3, pad).startswith(
        "igemm8_og2_splitk"), (cin, cout, size, ho)
    _conv_case(cin, cout, size, pad, dtype, n=n)


@pytest.mark.parametrize("cin,cout", [(128, 512), (128, 300)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv_g8_tail_split(cuda, cin, cout, dtype):
    """A full-K 256 x 256 grid of 1.41 rounds (362 tiles at 12 x 62^2 x 512 outputs, the SG3-T-256 L0-L2 shape at
    batch 32) runs as 256 full-K tiles + the 106 tail tiles split over K in two, the tail's partials combined over its
    pixels only (tile_base, p_lo): the plan picks it and the result matches F.conv2d in fp64 (partial o-tile: 300)."""
    dc = nv.F16 if dtype == torch.float16 else nv.BF16
    assert nv.conv_plan(dc, dc, nv.NHWC, 12, 62, 62, cin, nv.pad32(cout), cout, 3, 3, 1).startswith("igemm8_og2_tail")
    _conv_case(cin, cout, 62, 1, dtype, n=12)


@pytest.mark.parametrize("cin,cout,size,pad", [(128, 362, 88, 2), (96, 384, 81, 1)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv_split_384(cuda, cin, cout, size, pad, dtype):
    """cout_p 384 at a large M runs as two 8-phase launches (256-wide tile on channels 0-255, 128 x 512 tile on
    256-383, o_base): against F.conv2d in fp64, padded channels 362 -> 384 included."""
    _conv_case(cin, cout, size, pad, dtype, n=8)


@pytest.mark.parametrize("cin,cout,n,h,w", [(3, 32, 3, 67, 45), (3, 64, 2, 40, 33), (1, 32, 1, 9, 70), (4, 32, 2, 16, 32)])
def test_from_rgb_direct(cuda, cin, cout, n, h, w):
    """ic2_from_rgb_conv (from_rgb read straight from the NCHW f32 image, bf16 NHWC out) against F.conv2d in fp64
    on the same bf16-rounded operands, and against the packing + implicit-GEMM path it replaces (they differ
    only by f32 summation order: at most one bf16 rounding step apart)."""
    g = torch.Generator().manual_seed(cin * 100 + cout)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / np.sqrt(9 * cin))
        conv.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    x = torch.rand(n, cin, h, w, generator=g) * 2 - 1
    convg, xd = conv.to(cuda), x.to(cuda)
    stream = nv.stream_of(xd)
    from image_compression_2_amd import stylegan3_hvae_full as shf
    y = shf._from_rgb(convg, xd, torch.bfloat16, {}, stream)
    y_ref_path = shf._conv(convg, shf._to_nhwc(xd, torch.bfloat16, stream), torch.bfloat16, {}, stream)
    torch.cuda.synchronize()
    a = y.t[..., :cout].float().cpu().permute(0, 3, 1, 2)
    b = y_ref_path.t[..., :cout].float().cpu().permute(0, 3, 1, 2)
    r = F.conv2d(x.to(torch.bfloat16).double(), conv.weight.detach().cpu().to(torch.bfloat16).double(),
                 conv.bias.detach().cpu().double(), padding=1)
    assert (a.double() - r).abs().max().item() < 1e-2 * (1 + r.abs().max().item())
    assert (a - b).abs().max().item() <= 2 ** -7 * (1 + b.abs().max().item())
    assert torch.equal(y.t[..., cout:].cpu(), torch.zeros_like(y.t[..., cout:].cpu()))


@pytest.mark.parametrize("cin_p,n,size,pad", [(32, 2, 67, 0), (64, 1, 40, 0), (128, 3, 33, 0), (64, 2, 21, 1)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_torgb_1x1_nchw(cuda, cin_p, n, size, pad, dtype):
    """ToRGB (1x1 conv to 3 channels, bf16 / f16 NHWC in, NCHW f32 out with per-sample oscale, bias, clamp and
    out_mul: the SynthesisLayer L14 call) against an fp64 reference on the same operands."""
    g = torch.Generator().manual_seed(cin_p + size)
    x = (torch.randn(n, size, size, cin_p, generator=g) * 3).to(dtype)
    w = (torch.randn(32, cin_p, generator=g) / np.sqrt(cin_p)).to(dtype)
    osc = torch.rand(n, 32, generator=g) + 0.5
    bias = torch.randn(32, generator=g)
    so = size + 2 * pad  # a padded 1x1 (not the ToRGB kernel's shape) must take the implicit GEMM
    y = torch.empty(n, 3, so, so, device=cuda)
    xd, wd, od, bd = x.to(cuda), w.to(cuda), osc.to(cuda), bias.to(cuda)
    nv.conv_igemm(nv.ptr(xd), nv.ptr(wd), nv.ptr(y), nv.dtype_code(dtype), nv.F32, n, size, size, cin_p, 32, 3, 1, 1,
                  pad, so, so, nv.ptr(od), nv.ptr(bd), nv.ACT_LRELU, 1.0, 1.0, 8.0, 0.25, nv.NCHW, nv.stream_of(xd), cuda)
    torch.cuda.synchronize()
    xp = torch.nn.functional.pad(x.double(), (0, 0, pad, pad, pad, pad))
    acc = torch.einsum("nhwc,oc->nohw", xp, w.double()[:3])
    r = (acc * osc.double()[:, :3, None, None] + bias.double()[None, :3, None, None]).clamp(-8, 8) * 0.25
    assert _maxdiff(y, r) < 1e-4 * (1 + r.abs().max().item())


def _conv_case(cin, cout, size, pad, dtype=torch.bfloat16, n=3):
    cuda = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(cin + cout)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=pad)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / np.sqrt(9 * cin))
    x = torch.randn(n, cin, size, size, generator=g)
    convg = conv.to(cuda)
    stream = nv.stream_of(x.to(cuda))
    y = _to_nchw(_conv(convg, _to_nhwc(x.to(cuda), dtype, stream), dtype, {}, stream), stream)
    xr = x.to(dtype).float()
    wr = conv.weight.detach().cpu().to(dtype).float()
    r = F.conv2d(xr.double(), wr.double(), conv.bias.detach().cpu().double(), padding=pad)
    # bf16 / f16: one rounding of the stored output (2^-8 / 2^-11 relative) over the fp64 conv of the same operands
    tol = {torch.float32: 1e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}[dtype]
    assert _maxdiff(y, r) < tol * (1 + r.abs().max().item())


# ------------------------------------------------------------------ fully connected (fp32 reference)
@pytest.mark.parametrize("n,in_f,out_f,ldx,act", [(32, 512, 512, 512, 0), (40, 512, 7, 8192, 0), (3, 100, 33, 100, 1),
                                                  (5, 128, 256, 128, 1)])
def test_fc_matches_torch(cuda, n, in_f, out_f, ldx, act):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, ldx, generator=g)
    w = torch.randn(out_f, in_f, generator=g)
    b = torch.randn(out_f, generator=g)
    y = torch.empty(n, out_f, device=cuda)
    wg, bg = 1 / np.sqrt(in_f), 0.5
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)  # keep the device copies alive across the call
    nv.call("ic2_fc", nv.ptr(xd), ldx, nv.ptr(wd), nv.ptr(bd), nv.ptr(y), n, in_f, out_f,
            float(wg), bg, act, 0.2, float(np.sqrt(2)) if act else 1.0, nv.stream_of(y))
    torch.cuda.synchronize()
    r = (x[:, :in_f].double() @ w.double().t()) * wg + b.double() * bg
    if act:
        r = F.leaky_relu(r, 0.2) * np.sqrt(2)
    assert _maxdiff(y, r) < 1e-4 * (1 + r.abs().max().item())


# ------------------------------------------------------------------ GroupNorm + lrelu (+ pool), fp32 reference
@pytest.mark.parametrize("n,c,groups,h,w,pool", [(2, 64, 32, 5, 7, True), (3, 96, 32, 9, 6, False),
                                                 (32, 512, 32, 2, 2, True), (1, 32, 32, 40, 33, True),
                                                 (4, 128, 32, 64, 64, False), (2, 256, 32, 33, 31, False),
                                                 (2, 64, 32, 130, 128, True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_group_norm_lrelu_pool_matches_torch(cuda, n, c, groups, h, w, pool, dtype):
    from image_compression_2_amd.stylegan3_hvae_full import _group_norm_lrelu
    g = torch.Generator().manual_seed(6)
    x = torch.randn(n, c, h, w, generator=g) * 3 + 0.5
    norm = torch.nn.GroupNorm(groups, c)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(c, generator=g) + 0.5)
        norm.bias.copy_(torch.randn(c, generator=g))
    r = F.leaky_relu(norm(x), 0.2)
    if pool:
        r = F.avg_pool2d(r, 2)
    stream = nv.stream_of()
    xin = _to_nhwc(x.to(cuda), dtype, stream)
    out = _group_norm_lrelu(norm.to(cuda), xin, pool, dtype, stream)
    y = _to_nchw(out, stream)
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    assert _maxdiff(y, r) < tol * (1 + r.abs().max().item())


@pytest.mark.parametrize("cin,cout,n,h,w", [(32, 64, 2, 200, 181), (64, 64, 1, 257, 263), (3, 32, 2, 190, 200),
                                             (64, 32, 2, 181, 190), (96, 64, 1, 300, 230), (128, 128, 2, 64, 70),
                                             (32, 64, 1, 16, 20)])
@pytest.mark.parametrize("fuse", [0])
def test_conv3x3_gn_fwd_statistics(cuda, cin, cout, n, h, w, fuse):
    """ic2_conv3x3_gn_fwd in bf16: the conv output is the plain conv's, and the GroupNorm statistics (the
    separate pass; the halo conv's statistics epilogue, fuse=1, is gone) match ic2_group_norm_stats on the same stored
    output (fp64 partial sums, 1e-5 relative)."""
    from image_compression_2_amd.stylegan3_hvae_full import _conv_gn
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn(n, cin, h, w, generator=g)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(cuda)
    norm = torch.nn.GroupNorm(min(32, cout), cout).to(cuda)
    stream = nv.stream_of()
    xin = _to_nhwc(x.to(cuda), torch.bfloat16, stream)
    y_ref = _conv(conv, xin, torch.bfloat16, {}, stream)
    y, st = _conv_gn(conv, norm, xin, torch.bfloat16, {}, stream, fuse=fuse)
    assert torch.equal(y.t, y_ref.t)
    groups = norm.num_groups
    nfl = int(nv.query("ic2_group_norm_stats_floats", n, h * w, groups))
    ref = torch.empty([nfl], dtype=torch.float32, device=cuda)
    nv.call("ic2_group_norm_stats", nv.ptr(y.t), nv.BF16, n, h * w, y.c_p, cout, groups, float(norm.eps), nv.ptr(ref),
            stream)
    a, b = st[: n * groups * 2].view(-1, 2).cpu(), ref[: n * groups * 2].view(-1, 2).cpu()
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), (a - b).abs().max()
    # and against torch on the same rounded tensor
    yt = y.t.float()[..., :cout].permute(0, 3, 1, 2).reshape(n, groups, -1).double()
    assert torch.allclose(a[:, 0].double(), yt.mean(-1).reshape(-1).cpu(), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ metric / resize
@pytest.mark.parametrize("shape", [(3, 3, 16, 16), (2, 3, 7, 5), (1, 3, 256, 256)])
def test_uint8_sse_matches_reference_definition(cuda, shape):
    g = torch.Generator().manual_seed(4)
    a = torch.rand(*shape, generator=g) * 2.4 - 1.2
    b = torch.rand(*shape, generator=g) * 2 - 1
    sse = icm.uint8_sse(a.to(cuda), b.to(cuda)).cpu().numpy()
    assert np.array_equal(sse, om.sse_uint8(a, b))
    assert icm.psnr(a.to(cuda), b.to(cuda)) == pytest.approx(om.psnr(a, b), abs=1e-9)


def test_resize_bilinear(cuda):
    x = torch.randn(2, 3, 64, 64)
    y = ic2.resize_bilinear(x.to(cuda), (16, 16))
    r = F.interpolate(x, size=(16, 16), mode="bilinear", align_corners=False)
    assert _maxdiff(y, r) < 1e-5


@pytest.mark.parametrize("layer", [3, 7, 10, 13])
def test_flrelu_strip_segmentation_invariant(cuda, gen256_bf16_layers, layer):
    """The strip-streaming filtered lrelu cuts a strip into segments (one extra grid block each) only when a batch
    has too few strips to fill the chip.  Every grid block is computed from the same input rows with the same taps
    either way, so a batch of 16 at the layer's real channel count (whole strips) equals the same images run two
    at a time (segmented strips) bit for bit."""
    import ctypes
    L = gen256_bf16_layers[layer]
    n, c_p = 16, L.cout_p
    conv = int(L.in_size[0]) + 2
    s_out = int(L.out_size[0])
    g = torch.Generator().manual_seed(90 + layer)
    x = (torch.randn(n, c_p // 16, conv, conv, 16, generator=g) * 2).to(torch.float16).to(cuda)
    x[:, :, :3, :5] = 300.0
    ps = (torch.rand(n, c_p, generator=g) + 0.5).to(cuda)

    def run(xs, pss):
        out = torch.full((xs.shape[0], s_out, s_out, c_p), float("nan"), device=cuda, dtype=torch.bfloat16)
        nv.call("ic2_flrelu_nhwc16", nv.ptr(xs), nv.ptr(out), nv.F16, nv.BF16, xs.shape[0], c_p, conv, conv, s_out,
                s_out, L._fu.ctypes.data_as(ctypes.c_void_p), L._fu.shape[0], L._fd.ctypes.data_as(ctypes.c_void_p),
                L._fd.shape[0], None, L.up_factor, L.down_factor, *L.padding, float(np.sqrt(2)), 0.2, 256.0, 0,
                nv.ptr(pss), nv.stream_of(xs))
        return out

    full = run(x, ps)
    parts = torch.cat([run(x[i:i + 2].contiguous(), ps[i:i + 2].contiguous()) for i in range(0, n, 2)])
    torch.cuda.synchronize()
    assert torch.isfinite(full.float()).all()
    assert torch.equal(full, parts)


@pytest.mark.parametrize("layer", [10, 13])
def test_flrelu_strip_post_scale_rows_across_items(cuda, gen256_bf16_layers, layer):
    """the strip kernel DMAs each item's post-scale row (16 floats) into a 64-B LDS slot by four
    lanes of its last wave, together with the item's first input rows, while the previous item is still being
    computed.  Here every workgroup runs at least two items (n 4, 32 channels: more strips x segments than resident
    workgroups), up 4 (L10) and up 2 (L13), and the post-scale rows are distinct per sample and per channel, so a
    row that landed late, early or in the wrong slot shows up against the fp64 composition."""
    import ctypes
    L = gen256_bf16_layers[layer]
    n, c_p = 4, 32
    conv = int(L.in_size[0]) + 2
    s_out = int(L.out_size[0])
    tiles_x, tiles_y = -(-s_out // 32), -(-s_out // 16)
    strips = n * tiles_x * (c_p // 16)
    nseg = min(tiles_y, max(1, -(-2 * 512 // strips)))
    seg_len = -(-tiles_y // nseg)
    items = strips * -(-tiles_y // seg_len)
    assert items > 512, items   # > one item per resident workgroup (256 CUs x 2)
    g = torch.Generator().manual_seed(110 + layer)
    x = (torch.randn(n, c_p, conv, conv, generator=g) * 2).to(torch.float16).float()
    x[:, :, :3, :5] = 300.0
    ps = 0.5 + torch.arange(c_p, dtype=torch.float32)[None, :] / 16 + 0.37 * torch.arange(n, dtype=torch.float32)[:, None]
    xb = x.to(torch.float16).reshape(n, c_p // 16, 16, conv, conv).permute(0, 1, 3, 4, 2).contiguous().to(cuda)
    out = torch.full((n, s_out, s_out, c_p), float("nan"), device=cuda, dtype=torch.bfloat16)
    psd = ps.to(cuda)
    nv.call("ic2_flrelu_nhwc16", nv.ptr(xb), nv.ptr(out), nv.F16, nv.BF16, n, c_p, conv, conv, s_out, s_out,
            L._fu.ctypes.data_as(ctypes.c_void_p), L._fu.shape[0], L._fd.ctypes.data_as(ctypes.c_void_p),
            L._fd.shape[0], None, L.up_factor, L.down_factor, *L.padding, float(np.sqrt(2)), 0.2, 256.0, 0,
            nv.ptr(psd), nv.stream_of(xb))
    torch.cuda.synchronize()
    r = sg3.filtered_lrelu(x.double(), torch.from_numpy(L._fu).double(), torch.from_numpy(L._fd).double(), None,
                           up=L.up_factor, down=L.down_factor, padding=L.padding, gain=np.sqrt(2), slope=0.2,
                           clamp=256.0) * ps.double()[:, :, None, None]
    y = out.float().cpu().permute(0, 3, 1, 2).double()
    # per (sample, channel): the ratio of the output to the unscaled reference must be that row's scale
    err = ((y - r).abs().amax(dim=(2, 3)) / (1 + r.abs().amax(dim=(2, 3))))
    print(f"[flrelu post-scale rows L{layer}] items {items}, worst per-(n, c) relative error {err.max().item():.2e}")
    assert err.max().item() < 2e-2
