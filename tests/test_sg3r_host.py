"""CPU: the StyleGAN3-R configuration of the generator (radial down filters, 1x1 convs, twice the channels): filter
design, layer table, state-dict layout, the rank rule of the separable factorisation, the pickle loader's
allow_radial switch and the C ABI's argument checks.  The kernels are checked in tests/test_gpu_sg3r.py."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import sg3r_oracle as so
import test_legacy as tl
from image_compression_2_amd import _native as nv
from image_compression_2_amd import legacy
from image_compression_2_amd import networks_stylegan3 as ns
from image_compression_2_amd.networks_stylegan3 import Generator, SG3_R_KWARGS, SynthesisLayer
from oracle import sg3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(z_dim=32, w_dim=32, img_resolution=32, num_layers=6, channel_base=256, channel_max=24)


@pytest.fixture(scope="module")
def g256():
    torch.manual_seed(5)
    return Generator(img_resolution=256, **SG3_R_KWARGS)


@pytest.fixture(scope="module")
def g1024_layers():
    """R-1024's layers without its 1024-wide weights' mapping network: the synthesis alone."""
    torch.manual_seed(6)
    kw = {k: v for k, v in SG3_R_KWARGS.items()}
    return ns.SynthesisNetwork(w_dim=512, img_resolution=1024, img_channels=3, **kw)


def test_r_kwargs_constant():
    assert SG3_R_KWARGS == dict(conv_kernel=1, channel_base=65536, channel_max=1024, use_radial_filters=True)


@pytest.mark.parametrize("idx", [0, 2, 9])
def test_radial_design_properties(g256, idx):
    L = g256.synthesis.layers()[idx]
    _, table = sg3.layer_table(256, **so.R_TABLE_KW)
    assert L.down_radial and L.down_filter.shape == (12, 12) and L.down_filter.dtype == torch.float32
    f = L.down_filter.numpy()
    assert L._fd.shape == (12, 12) and np.array_equal(L._fd, f)
    assert abs(float(f.sum(dtype=np.float32)) - 1) < 1e-6
    assert np.array_equal(f, f.T) and np.array_equal(f, f[::-1, ::-1])
    ref = so.layer_design(table[idx])
    assert np.abs(f - ref).max() < 1e-7
    # radial symmetry under the separable window: f / outer(w, w) depends on i^2 + j^2 alone
    w = so.kaiser_window(12, table[idx]["out_half_width"] * 2, table[idx]["tmp_sampling_rate"])
    q = f.astype(np.float64) / np.outer(w, w)
    i = np.arange(12) * 2 - 11
    r2 = i[:, None] ** 2 + i[None, :] ** 2
    scale = np.abs(q).max()
    for v in np.unique(r2):
        vals = q[r2 == v]
        assert np.ptp(vals) < 1e-5 * scale, (v, vals)   # float32 storage of f
    assert (r2 == 50).sum() == 12     # radii shared beyond the mirror images count too: 1^2 + 7^2 = 5^2 + 5^2


def test_critical_layers_and_torgb_keep_t_filters(g256):
    _, table = sg3.layer_table(256, **so.R_TABLE_KW)
    for L, T in list(zip(g256.synthesis.layers(), table))[-3:]:
        assert not L.down_radial and L.down_rank == 0
        if T["down_filter"] is None:
            assert L.down_filter is None
        else:
            assert L.down_filter.ndim == 1 and torch.equal(L.down_filter, T["down_filter"])
    for L, T in zip(g256.synthesis.layers(), table):   # up filters stay separable everywhere
        assert (L.up_filter is None) == (T["up_filter"] is None)
        if L.up_filter is not None:
            assert torch.equal(L.up_filter, T["up_filter"])
        assert L.padding == T["padding"] and L.up_factor == T["up"] and L.down_factor == T["down"]
        assert L.unread_border() == 0 if not L.is_torgb else True


def test_layer_names(g256, g1024_layers):
    assert g256.synthesis.layer_names == so.R256_NAMES
    assert g1024_layers.layer_names == so.R1024_NAMES
    assert g256.num_ws == 16 and g256.w_dim == 512


def test_make_generator_r():
    G = ns.make_generator(256, seed=3, device="cpu", **SG3_R_KWARGS)
    assert G.synthesis.layer_names == so.R256_NAMES and G.synthesis.input.channels == 1024
    assert not any(p.requires_grad for p in G.parameters())


def test_state_dict_matches_oracle_layout(g256):
    sd = g256.state_dict()
    ref = so.patch_state_dict(sg3.init_params(256, **so.R_TABLE_KW), 256, **so.R_TABLE_KW)
    assert set(sd) == set(ref)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
    radial = so.radial_designs(256, **so.R_TABLE_KW)
    assert sorted(radial) == sorted(so.R256_NAMES[:12])
    for name in so.R256_NAMES:
        f = sd.get(f"synthesis.{name}.down_filter")
        assert (f is not None and f.ndim == 2) == (name in radial), name
        if name in radial:
            assert (f - ref[f"synthesis.{name}.down_filter"]).abs().max() < 1e-7


def test_rank_rule_on_every_radial_layer(g256, g1024_layers):
    seen = set()
    for syn in (g256.synthesis, g1024_layers):
        for L in syn.layers():
            if not L.down_radial:
                continue
            r_ref, err = so.rank_rule(L._fd)
            assert L.down_rank == r_ref and L.down_rank in (2, 3)
            fr = L._fdv.astype(np.float64).T @ L._fdh.astype(np.float64)
            assert L._fdv.shape == L._fdh.shape == (L.down_rank, 12) and L._fdv.dtype == np.float32
            bound = np.abs(L._fd.astype(np.float64)).sum() / 2048
            # the factors are stored in float32: 2 * 12 * 12 roundings of 2^-24 relative on top of the bound
            assert np.abs(L._fd - fr).sum() <= bound + 1e-5
            assert err <= bound
            seen.add(L.down_rank)
    assert seen == {2, 3}


def test_rank_rule_sends_a_full_rank_filter_to_the_direct_kernel():
    f = np.random.default_rng(0).standard_normal((12, 12))
    assert so.rank_rule(f)[0] > 4
    assert ns.radial_rank(f) == (0, None, None)
    # and an exactly separable one is rank 1
    r, fv, fh = ns.radial_rank(np.outer(np.arange(1, 13), np.arange(2, 14)) / 100.0)
    assert r == 1 and fv.shape == fh.shape == (1, 12)


def test_blocked_output_is_decided_by_down_radial_not_by_shape(g256):
    L0, L12 = g256.synthesis.layers()[0], g256.synthesis.layers()[12]
    assert L0.down_radial and L0.writes_blocked_output(torch.float16) and not L0.writes_blocked_output(torch.float32)
    assert not L12.down_radial and L12.writes_blocked_output(torch.bfloat16)
    L0.down_radial = False     # a [12, 12] array must not pass for 12 separable taps
    try:
        assert not L0.writes_blocked_output(torch.float16)
    finally:
        L0.down_radial = True


def _r_init_kwargs():
    kw = dict(SMALL, mapping_kwargs={"num_layers": 2}, c_dim=0, img_channels=3)
    kw.update(conv_kernel=1, use_radial_filters=True)
    return kw


def test_legacy_allow_radial_round_trip():
    torch.manual_seed(3)
    G = Generator(**SMALL, conv_kernel=1, use_radial_filters=True)
    with torch.no_grad():
        for k, b in G.named_buffers():
            if k.endswith("magnitude_ema"):
                b.fill_(0.37)
        G.mapping.w_avg.normal_()
    blob = tl._write_pkl(G, _r_init_kwargs())
    with pytest.raises(NotImplementedError):
        legacy.load_network_pkl(io.BytesIO(blob), device="cpu")
    rec = legacy.SafeUnpickler(io.BytesIO(blob)).load()["G_ema"]
    with pytest.raises(NotImplementedError):
        legacy.generator_from_record(rec, device="cpu")
    G2 = legacy.load_network_pkl(io.BytesIO(blob), device="cpu", allow_radial=True)["G_ema"]
    assert isinstance(G2, Generator)
    sd, sd2 = G.state_dict(), G2.state_dict()
    assert list(sd) == list(sd2)
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
    assert [n for n, _ in G2.synthesis.named_children()] == [n for n, _ in G.synthesis.named_children()]
    assert [L.down_radial for L in G2.synthesis.layers()] == [True] * 4 + [False] * 3
    assert legacy.generator_from_record(rec, device="cpu", allow_radial=True).synthesis.layer_names == \
        G.synthesis.layer_names


def test_legacy_t_state_dict_under_r_kwargs_fails_strictly():
    torch.manual_seed(3)
    G_t = Generator(**SMALL, conv_kernel=1)    # same keys, 1-D down filters
    blob = tl._write_pkl(G_t, _r_init_kwargs())
    with pytest.raises(RuntimeError, match="down_filter"):
        legacy.load_network_pkl(io.BytesIO(blob), device="cpu", allow_radial=True)


def test_entry_point_index_names_the_2d_entry_points():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    listed = set(re.findall(r"`(ic2_[a-z0-9_]+)`", doc))
    hdr = open(os.path.join(ROOT, "include", "ic2ops.h")).read()
    for name in ("ic2_flrelu_nhwc_2d", "ic2_flrelu_nhwc16_2d"):
        assert name in listed and name in nv.exported_symbols() and re.search(r"\b%s\(" % name, hdr)
    assert nv.load().ic2_abi_version() == 1


def _call_2d(name="ic2_flrelu_nhwc_2d", **over):
    """One call of a 2-D entry point on a valid 8 x 8 x 16 problem with `over` applied -> (code, message).  The tensors
    are real device buffers where a GPU exists (a check that wrongly passed would then launch on valid memory) and
    dummy non-null addresses elsewhere (no device: nothing can launch)."""
    fu = np.full(12, 1 / 12, np.float32)
    fd = np.full((12, 12), 1 / 144, np.float32)
    if torch.cuda.is_available():
        bufs = [torch.zeros(1, 8, 8, 16, device="cuda") for _ in range(2)]
        x, y = (ctypes.c_void_p(t.data_ptr()) for t in bufs)
    else:
        x = y = ctypes.c_void_p(16)
    a = dict(x=x, y=y, din=nv.F32, dout=nv.F32, n=1, c_p=16, in_h=8, in_w=8,
             out_h=8, out_w=8, fu=fu, fu_taps=12, fd=fd, fd_taps=12, rank=0, fdv=None, fdh=None, up=2, down=2,
             pad=(11, 10, 11, 10))
    a.update(over)
    fp = lambda v: None if v is None else v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib = nv.load()
    rc = getattr(lib, name)(a["x"], a["y"], a["din"], a["dout"], a["n"], a["c_p"], a["in_h"], a["in_w"], a["out_h"],
                            a["out_w"], fp(a["fu"]), a["fu_taps"], fp(a["fd"]), a["fd_taps"], a["rank"], fp(a["fdv"]),
                            fp(a["fdh"]), None, a["up"], a["down"], *a["pad"], 1.0, 0.2, -1.0, 0, None, None)
    return rc, lib.ic2_last_error().decode()


def test_2d_entry_point_refuses_before_any_launch():
    """Every refusal below returns before a kernel could be launched: the tensor pointers are not device memory."""
    assert _call_2d(x=None)[0] == 1
    rc, msg = _call_2d(rank=5, fdv=np.zeros((5, 12), np.float32), fdh=np.zeros((5, 12), np.float32))
    assert rc == 1 and "rank" in msg
    rc, msg = _call_2d(rank=2)
    assert rc == 1 and "tap vectors" in msg
    rc, msg = _call_2d(fd_taps=13)
    assert rc == 1 and "taps" in msg
    rc, msg = _call_2d(out_h=9)
    assert rc == 1 and "expected 8x8" in msg
    rc, msg = _call_2d(pad=(11, 10, 10, 11))
    assert rc == 2 and "mod up" in msg
    rc, msg = _call_2d(c_p=24)
    assert rc == 1
    rc, msg = _call_2d(din=nv.BF16, dout=nv.F16)
    assert rc == 1 and "dtype pair" in msg
    rc, msg = _call_2d(name="ic2_flrelu_nhwc16_2d")
    assert rc == 1 and "16-bit" in msg
    rc, msg = _call_2d(dout=nv.F32 | nv.flr_out_layout(nv.NHWC16))
    assert rc == 1 and "16-bit" in msg
    # a geometry without an instance: up 1
    rc, msg = _call_2d(up=1, fu_taps=1, fu=np.ones(1, np.float32), pad=(5, 6, 5, 6), in_h=16, in_w=16)
    assert rc == 2 and "no fused instance" in msg


def test_autograd_refusal_needs_no_gpu():
    """The raise comes before any launch, so it is reachable on the CPU: the same call on a T generator gets as far as
    the native path's device check."""
    torch.manual_seed(0)
    G = Generator(**SMALL, conv_kernel=1, use_radial_filters=True).eval().requires_grad_(False)
    ws = torch.randn(2, G.num_ws, G.w_dim, requires_grad=True)
    with pytest.raises(nv.AutogradUnsupported, match="StyleGAN3-R"):
        G.synthesis(ws)
    L = G.synthesis.layers()[0]
    x = torch.randn(2, L.in_channels, 36, 36, requires_grad=True)
    with pytest.raises(nv.AutogradUnsupported, match="StyleGAN3-R"):
        L(x, torch.randn(2, G.w_dim))
    assert isinstance(L, SynthesisLayer)
