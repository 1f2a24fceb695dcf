"""GPU: the StyleGAN3-R configuration.  ic2_flrelu_nhwc_2d / ic2_flrelu_nhwc16_2d (filtered lrelu with a 2-D down
filter, csrc/flrelu_radial.hip) per element against the fp64 oracle composition (oracle/sg3.py filtered_lrelu with a
2-D fd), the 1x1 modulated conv layer, and R generators end to end against oracle.sg3.synthesis_forward on a state
dict whose radial layers carry the 2-D design (tests/sg3r_oracle.py).

Every output is NaN-prefilled and sits between sentinel guard bands, so an unwritten element or a store outside the
tensor fails the test."""
import ctypes

import numpy as np
import pytest
import torch

import image_compression_2_amd as ic2
import sg3r_oracle as so
from image_compression_2_amd import _native as nv
from image_compression_2_amd import networks_stylegan3 as ns
from oracle import sg3

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -1234.5
GAIN, SLOPE, CLAMP = float(np.sqrt(2)), 0.2, 256.0
# (up, padding, in_h, in_w): the R layers' two geometries on sizes that are no multiple of a tile
GEOMS = {2: (2, [11, 10, 11, 10], 23, 38), 4: (4, [-2, -5, -2, -5], 21, 19)}


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


def _fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _out_size(in_h, in_w, up, pad, tu=None, td=12):
    tu = 6 * up if tu is None else tu
    return sg3.filtered_lrelu_out_size(in_h, in_w, tu, td, up, 2, pad)


def _guarded(shape, dtype, cuda):
    """(base, view): a NaN-prefilled tensor of `shape` inside a buffer with GUARD sentinels on both sides."""
    numel = int(np.prod(shape))
    base = torch.full([GUARD + numel + GUARD], SENTINEL, device=cuda, dtype=dtype)
    base[GUARD:GUARD + numel] = float("nan")
    view = base[GUARD:GUARD + numel].view(shape)
    assert view.data_ptr() % 16 == 0
    return base, view


def _guards_intact(base):
    b = base.cpu()
    return bool((b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all())


def _to_layout(x_nchw, dtype, blocked, cuda):
    """NCHW CPU tensor -> NHWC, or channel-blocked [n, c/16, h, w, 16], on the device."""
    n, c, h, w = x_nchw.shape
    x = x_nchw.permute(0, 2, 3, 1)
    if blocked:
        x = x.reshape(n, h, w, c // 16, 16).permute(0, 3, 1, 2, 4)
    return x.contiguous().to(cuda, dtype)


def _from_layout(y, blocked):
    """Device output -> NCHW CPU tensor (same dtype)."""
    y = y.cpu()
    if blocked:
        n, cb, h, w, _ = y.shape
        return y.permute(0, 1, 4, 2, 3).reshape(n, cb * 16, h, w)
    return y.permute(0, 3, 1, 2)


def _call(cuda, x, in_dtype, out_dtype, fu, fd, up, pad, bias=None, ps=None, flip=False, in_blocked=False,
          out_blocked=False, rank=0, fdv=None, fdh=None, expect=0, out_hw=None):
    """Runs a 2-D entry point on x (NCHW CPU tensor) -> (code, output as an NCHW CPU tensor, guards intact?)."""
    n, c_p, in_h, in_w = x.shape
    oh, ow = _out_size(in_h, in_w, up, pad, fu.shape[0], fd.shape[0]) if out_hw is None else out_hw
    xd = _to_layout(x, in_dtype, in_blocked, cuda)
    shape = [n, c_p // 16, oh, ow, 16] if out_blocked else [n, oh, ow, c_p]
    base, out = _guarded(shape, out_dtype, cuda)
    bd = None if bias is None else bias.to(cuda)
    psd = None if ps is None else ps.to(cuda)
    lib = nv.load()
    fn = lib.ic2_flrelu_nhwc16_2d if in_blocked else lib.ic2_flrelu_nhwc_2d
    rc = fn(nv.ptr(xd), nv.ptr(out), nv.dtype_code(in_dtype),
            nv.dtype_code(out_dtype) | (nv.flr_out_layout(nv.NHWC16) if out_blocked else 0), n, c_p, in_h, in_w, oh, ow,
            _fp(fu), fu.shape[0], _fp(fd), fd.shape[0], rank, _fp(fdv), _fp(fdh), nv.ptr(bd), up, 2, *pad, GAIN, SLOPE,
            CLAMP, int(flip), nv.ptr(psd), nv.stream_of(xd))
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.ic2_last_error().decode())
    return rc, _from_layout(out, out_blocked), _guards_intact(base)


def _ref(x, fu, fd, up, pad, bias=None, ps=None, flip=False):
    r = sg3.filtered_lrelu(x.double(), torch.from_numpy(fu).double(), torch.from_numpy(fd).double(),
                           None if bias is None else bias.double(), up=up, down=2, padding=pad, gain=GAIN, slope=SLOPE,
                           clamp=CLAMP, flip_filter=flip)
    return r if ps is None else r * ps.double()[:, :, None, None]


def _nonsym_filters(up, seed):
    """A non-symmetric separable up filter and a non-symmetric full-rank 12 x 12 down filter with unit DC gain: the
    real filters are symmetric and would hide a transposed or unflipped tap table."""
    rng = np.random.default_rng(seed)
    fu = sg3.design_lowpass_filter(6 * up, 8.0, 4.0, 64).numpy().astype(np.float64) * (1 + 0.4 * rng.random(6 * up))
    fd = rng.standard_normal((12, 12)) * 0.3 + np.outer(np.hanning(14)[1:-1], np.hanning(14)[1:-1])
    fd /= fd.sum()
    assert not np.allclose(fd, fd.T) and not np.allclose(fd, fd[::-1, ::-1])
    return np.ascontiguousarray(fu / fu.sum(), np.float32), np.ascontiguousarray(fd, np.float32)


def _input(n, c_p, in_h, in_w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c_p, in_h, in_w, generator=g) * 2
    x[:, :, :3, :5] = 300.0   # exercises the clamp
    return x, torch.randn(c_p, generator=g), torch.rand(n, c_p, generator=g) + 0.5


# ------------------------------------------------------------------ 1. direct kernel, f32
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "bias_ps"])
@pytest.mark.parametrize("c_p", [16, 48])
@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("up", [2, 4])
def test_direct_f32_matches_fp64(cuda, up, flip, c_p, extras):
    up, pad, in_h, in_w = GEOMS[up]
    fu, fd = _nonsym_filters(up, 3)
    x, b, ps = _input(2, c_p, in_h, in_w, 40 + up)
    b, ps = (b, ps) if extras else (None, None)
    _, y, ok = _call(cuda, x, torch.float32, torch.float32, fu, fd, up, pad, bias=b, ps=ps, flip=flip)
    r = _ref(x, fu, fd, up, pad, bias=b, ps=ps, flip=flip)
    assert ok, "store outside the output tensor"
    assert y.shape == r.shape == (2, c_p) + tuple(_out_size(in_h, in_w, up, pad))
    assert torch.isfinite(y).all(), "an output element was not written"
    err = (y.double() - r).abs().max().item()
    print(f"max|diff| {err:.3e}  max|ref| {r.abs().max().item():.3e}")
    assert err < 2e-5 * (1 + r.abs().max().item())


# ------------------------------------------------------------------ 2. 16-bit pairs
PAIRS = [(torch.float16, torch.float16), (torch.float16, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]
PAIR_IDS = ["f16_f16", "f16_bf16", "bf16_bf16"]
_layer_cache = {}


def _r256_filters(name):
    """(up, padding, fu, fd, rank, fdv, fdh) of an R-256 layer, or of the non-symmetric full-rank filter."""
    if name == "nonsym":
        fu, fd = _nonsym_filters(2, 5)
        assert ns.radial_rank(fd)[0] == 0   # full rank: no factorisation offered, the direct kernel
        return 2, GEOMS[2][1], fu, fd, 0, None, None
    if not _layer_cache:
        _, table = sg3.layer_table(256, **so.R_TABLE_KW)
        _layer_cache.update({L["name"].split("_")[0]: L for L in table})
    L = _layer_cache[name]
    fd = np.ascontiguousarray(so.layer_design(L), np.float32)
    rank, fdv, fdh = ns.radial_rank(fd)
    assert L["padding"] == GEOMS[L["up"]][1]
    return (L["up"], L["padding"], np.ascontiguousarray(L["up_filter"].numpy(), np.float32), fd, rank, fdv, fdh)


_ref16_cache = {}


def _case16(name, in_dtype):
    """Input, post_scale and fp64 reference on the rounded input: computed once per (filter, input dtype)."""
    key = (name, in_dtype)
    if key not in _ref16_cache:
        up, pad, fu, fd, rank, fdv, fdh = _r256_filters(name)
        _, _, in_h, in_w = GEOMS[up]
        x, _, ps = _input(2, 32, in_h, in_w, 60 + up)
        x = x.to(in_dtype).float()
        _ref16_cache[key] = (x, ps, _ref(x, fu, fd, up, pad, ps=ps))
    return _ref16_cache[key]


@pytest.mark.parametrize("out_blocked", [False, True], ids=["out_nhwc", "out_nhwc16"])
@pytest.mark.parametrize("in_blocked", [False, True], ids=["in_nhwc", "in_nhwc16"])
@pytest.mark.parametrize("name,want_rank", [("L0", 2), ("L3", 2), ("L9", 3), ("nonsym", 0)])
@pytest.mark.parametrize("in_dtype,out_dtype", PAIRS, ids=PAIR_IDS)
def test_16bit_pairs_match_fp64(cuda, in_dtype, out_dtype, name, want_rank, in_blocked, out_blocked):
    up, pad, fu, fd, rank, fdv, fdh = _r256_filters(name)
    assert rank == want_rank and (name != "L3" or up == 4)
    x, ps, r = _case16(name, in_dtype)
    _, y, ok = _call(cuda, x, in_dtype, out_dtype, fu, fd, up, pad, ps=ps, in_blocked=in_blocked,
                     out_blocked=out_blocked, rank=rank, fdv=fdv, fdh=fdh)
    assert ok, "store outside the output tensor"
    assert y.shape == r.shape and y.dtype == out_dtype
    assert torch.isfinite(y).all(), "an output element was not written"
    err = (y.double() - r).abs()
    scale = r.abs().max().item()
    print(f"max {err.max().item():.3e} mean {err.mean().item():.3e}  max|ref| {scale:.3e} "
          f"mean|ref| {r.abs().mean().item():.3e}")
    assert err.max().item() < 2e-2 * (1 + scale), (err.max().item(), scale)
    assert err.mean().item() < 2e-3 * (1 + r.abs().mean().item())
    if out_dtype == torch.float16:
        assert err.max().item() < 4e-3 * (1 + scale), (err.max().item(), scale)


# ------------------------------------------------------------------ 3. layout equalities
@pytest.mark.parametrize("name", ["L0", "L3"])
@pytest.mark.parametrize("in_dtype,out_dtype", PAIRS, ids=PAIR_IDS)
def test_layouts_give_the_same_bits(cuda, in_dtype, out_dtype, name):
    up, pad, fu, fd, rank, fdv, fdh = _r256_filters(name)
    x, ps, _ = _case16(name, in_dtype)
    kw = dict(ps=ps, rank=rank, fdv=fdv, fdh=fdh)
    _, base, _ = _call(cuda, x, in_dtype, out_dtype, fu, fd, up, pad, **kw)
    for in_blocked, out_blocked in ((True, False), (False, True), (True, True)):
        _, y, ok = _call(cuda, x, in_dtype, out_dtype, fu, fd, up, pad, in_blocked=in_blocked, out_blocked=out_blocked,
                         **kw)
        assert ok and torch.equal(y.view(torch.int16), base.view(torch.int16)), (in_blocked, out_blocked)


# ------------------------------------------------------------------ 4. refusals
def test_refusals_write_nothing(cuda):
    up, pad, in_h, in_w = GEOMS[2]
    fu, fd = _nonsym_filters(2, 3)
    x, _, _ = _input(1, 16, in_h, in_w, 7)
    oh, ow = _out_size(in_h, in_w, up, pad)
    fv = np.zeros((5, 12), np.float32)
    cases = [
        dict(pad=[11, 10, 10, 11], expect=2),                                      # px0 != py0 (mod up)
        dict(out_hw=(oh, ow + 1), expect=1),                                       # wrong output size
        dict(fd=np.zeros((13, 13), np.float32), out_hw=(oh, ow), expect=1),        # fd_taps above the cap
        dict(rank=5, fdv=fv, fdh=fv, expect=1),                                    # rank above 4
        dict(rank=2, expect=1),                                                    # rank without its vectors
    ]
    for dt in (torch.float32, torch.float16):
        for c in cases:
            kw = dict(pad=pad, fd=fd)
            kw.update(c)
            p, f = kw.pop("pad"), kw.pop("fd")
            rc, y, ok = _call(cuda, x, dt, dt, fu, f, up, p, **kw)
            assert rc != 0 and ok and torch.isnan(y).all(), c
    # the channel-blocked layouts are 16-bit only
    rc, y, ok = _call(cuda, x, torch.float32, torch.float32, fu, fd, up, pad, out_blocked=True, expect=1)
    assert ok and torch.isnan(y).all()


# ------------------------------------------------------------------ 5. the 1x1 modulated conv layer (unbatched modulation)
def test_1x1_layer_520_channels_matches_oracle(cuda):
    torch.manual_seed(12)
    cin, cout, w_dim, s = 520, 40, 32, 10
    L = ic2.SynthesisLayer(w_dim=w_dim, is_torgb=False, is_critically_sampled=False, use_fp16=False, in_channels=cin,
                           out_channels=cout, in_size=s, out_size=s, in_sampling_rate=16, out_sampling_rate=16,
                           in_cutoff=4.0, out_cutoff=4.5, in_half_width=3.0, out_half_width=2.8, conv_kernel=1,
                           use_radial_filters=True)
    assert L.down_radial and not L.batchable() and L.padding == [11, 10, 11, 10] and L.up_factor == 2
    with torch.no_grad():
        L.bias.normal_()
        L.magnitude_ema.fill_(0.6)
    L = L.to(cuda).eval()
    sd = {"synthesis.L." + k: v.detach().float().cpu() for k, v in L.state_dict().items()}
    assert sd["synthesis.L.down_filter"].shape == (12, 12)
    spec = dict(name="L", is_torgb=False, in_channels=cin, conv_kernel=1, up=2, down=2, padding=L.padding)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, cin, s, s, generator=g)
    w = torch.randn(2, w_dim, generator=g)
    y = L(x.to(cuda), w.to(cuda))
    r = sg3.synthesis_layer(sd, spec, x.double(), w.double(), dtype=torch.float64)
    assert y.shape == r.shape == (2, cout, s, s)
    err = (y.cpu().double() - r).abs().max().item()
    print(f"max|diff| {err:.3e}  max|ref| {r.abs().max().item():.3e}")
    assert err < 1e-4 * (1 + r.abs().max().item())    # test_gpu_path.py::test_synthesis_layer_api_matches_oracle's bar


# ------------------------------------------------------------------ 6. end to end
SMALL = dict(z_dim=32, w_dim=32, img_resolution=32, num_layers=6, channel_base=256, channel_max=24)
WIDE = dict(z_dim=64, w_dim=64, img_resolution=32, num_layers=6, channel_base=2560, channel_max=640)
_e2e_cache = {}


def _table_kw(cfg, conv_kernel):
    return dict(num_layers=cfg["num_layers"], channel_base=cfg["channel_base"], channel_max=cfg["channel_max"],
                conv_kernel=conv_kernel)


def _e2e(cuda, cfg_name, radial):
    """(generator on the device, ws, fp64 oracle image): built once per configuration."""
    key = (cfg_name, radial)
    if key not in _e2e_cache:
        cfg = dict(SMALL if cfg_name == "small" else WIDE)
        torch.manual_seed(21)
        kw = dict(conv_kernel=1, use_radial_filters=True) if radial else {}
        G = ic2.Generator(**cfg, **kw).eval().requires_grad_(False)
        ws = torch.randn(2, G.num_ws, G.w_dim, generator=torch.Generator().manual_seed(3)) * 0.7
        sd = {k: v.detach().float().cpu() for k, v in G.state_dict().items()}
        tkw = _table_kw(cfg, 1 if radial else 3)
        if radial:   # the recipe: the oracle reads the 2-D design from the state dict
            mine = {k: v.clone() for k, v in sd.items() if k.endswith("down_filter")}
            so.patch_state_dict(sd, cfg["img_resolution"], **tkw)
            for k, v in mine.items():
                assert v.shape == sd[k].shape and (v - sd[k]).abs().max() < 1e-7, k
        ref = sg3.synthesis_forward(sd, cfg["img_resolution"], ws, dtype=torch.float64, **tkw)
        _e2e_cache[key] = (G.to(cuda), ws, ref)
    return _e2e_cache[key]


def _e2e_err(cuda, cfg_name, radial, precision):
    G, ws, ref = _e2e(cuda, cfg_name, radial)
    G.set_precision(precision)
    img = G.synthesis(ws.to(cuda), noise_mode="const")
    assert img.shape == ref.shape and img.dtype == torch.float32 and torch.isfinite(img).all()
    return (img.cpu().double() - ref).abs().max().item()


@pytest.mark.parametrize("cfg_name", ["small", "wide"])
def test_r_synthesis_fp32_within_1e3_of_oracle(cuda, cfg_name):
    G, _, _ = _e2e(cuda, cfg_name, True)
    layers = G.synthesis.layers()
    assert [int(L.out_size[0]) for L in layers[:-1]] == [36, 36, 52, 52, 52, 32]
    assert {L.up_factor for L in layers if L.down_radial} == {2, 4}
    assert {L.down_rank for L in layers if L.down_radial} == {2, 3}
    if cfg_name == "wide":
        assert G.synthesis.layer_names[0] == "L0_36_640" and G.synthesis.input.channels == 640
        assert not all(L.batchable() for L in layers)
    err = _e2e_err(cuda, cfg_name, True, "fp32")
    print(f"{cfg_name}: fp32 max|err| {err:.3e}")
    assert err < 1e-3


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_r_synthesis_16bit_within_2x_of_t(cuda, precision):
    """The 16-bit R synthesis against the fp64 oracle, next to the T generator of the same small shape (conv_kernel 3,
    separable filters: existing code, the baseline).  R must stay within 2x of T's error: the margin covers the
    different channel counts per layer.  Measured values: profiles/r16_sg3r.txt."""
    e_r = _e2e_err(cuda, "small", True, precision)
    e_t = _e2e_err(cuda, "small", False, precision)
    e_w = _e2e_err(cuda, "wide", True, precision)
    print(f"{precision}: max|err| R small {e_r:.3e}  T small {e_t:.3e}  R wide {e_w:.3e}")
    assert e_r <= 2 * e_t, (e_r, e_t)


def test_r_compressor_and_evaluation_run(cuda):
    G, _, _ = _e2e(cuda, "small", True)
    G.set_precision("fp32")
    torch.manual_seed(7)
    enc = ic2.HVAE_VGG_Encoder(img_resolution=64, w_dim=G.w_dim, num_ws=G.num_ws, block_split=(3, 6), channel_base=256,
                               channel_max=32).to(cuda)
    comp = ic2.StyleGAN3Compressor(enc, G, training_resolution=64)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(cuda)
    q = comp.compress(x, quantization_bits=8)
    assert q.shape == (2, G.num_ws, G.w_dim)
    img = comp.decompress(q)
    assert img.shape == (2, 3, 32, 32) and torch.isfinite(img).all()
    assert torch.equal(img, G.synthesis(q))
    rec = ic2.evaluate_compression(comp, x, quantization_bits=8)
    assert rec["n_images"] == 2 and np.isfinite(rec["batch_psnr_quantized"]) and np.isfinite(rec["batch_ssim_quantized"])
    assert rec["compressed_size_bytes"] == G.num_ws * G.w_dim


# ------------------------------------------------------------------ 7. autograd refusal
def test_r_synthesis_refuses_autograd(cuda):
    G, ws, _ = _e2e(cuda, "small", True)
    with torch.enable_grad():
        w = ws.to(cuda).requires_grad_()
        with pytest.raises(nv.AutogradUnsupported, match="StyleGAN3-R"):
            G.synthesis(w)
