"""CPU: the host side of training through the Gumbel-softmax quantizer (the reference's
train_gumbel_discretized_hvae, gumbel_softmax_compression.py:322-611): argument validation of the new entry points
before any launch, the no-fallback rule in training mode, and train_step_gumbel's defaults."""
import ctypes
import inspect

import pytest
import torch

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from image_compression_2_amd import training as ict

F = ctypes.c_void_p(16)   # a non-null pointer that is never dereferenced: validation fails before any launch


def _bwd(z=F, n=8, cb=F, k=256, seed=F, noise=None, g=F, dz=F, dlogt=None, ws=None, ws_bytes=0):
    return nv.query("ic2_gumbel_softmax_quantize_bwd", z, n, cb, k, F, 1.0, seed, 0, noise, g, None, dz, dlogt, ws,
                    ws_bytes, None)


@pytest.mark.parametrize("k", [0, 2000])
def test_gumbel_backward_rejects_codebook_sizes(k):
    lib = nv.load()
    assert _bwd(k=k) == 1
    assert b"gumbel_softmax_quantize_bwd" in lib.ic2_last_error() and str(k).encode() in lib.ic2_last_error()
    assert nv.query("ic2_gumbel_noise", F, 0, 0, 8, k, F, None) == 1
    assert b"gumbel_noise" in lib.ic2_last_error() and str(k).encode() in lib.ic2_last_error()


def test_gumbel_backward_rejects_null_pointers():
    lib = nv.load()
    assert _bwd(z=None) == 1
    assert b"null pointer" in lib.ic2_last_error()
    assert _bwd(dz=None) == 1
    assert _bwd(g=None) == 1
    assert nv.query("ic2_gumbel_noise", F, 0, 0, 8, 256, None, None) == 1
    assert b"null pointer" in lib.ic2_last_error()


def test_gumbel_backward_needs_a_seed_or_noise():
    lib = nv.load()
    assert _bwd(seed=None, noise=None) == 1
    assert b"seed_dev" in lib.ic2_last_error() and b"gumbel_noise" in lib.ic2_last_error()


def test_gumbel_backward_temperature_gradient_needs_its_workspace():
    """dlog tau is reduced through a caller-owned workspace of ic2_gumbel_softmax_bwd_ws_bytes(n): one f32 per
    workgroup, 4 latents (waves) per workgroup, at most 4096 workgroups."""
    lib = nv.load()
    ws_bytes = lambda n: nv.query("ic2_gumbel_softmax_bwd_ws_bytes", n)
    assert [ws_bytes(n) for n in (0, 1, 4, 5, 301, 16384, 16385, 1 << 40)] == [0, 4, 4, 8, 304, 16384, 16384, 16384]
    assert _bwd(n=301, dlogt=F, ws=F, ws_bytes=300) == 1
    assert b"workspace" in lib.ic2_last_error() and b"304" in lib.ic2_last_error()
    assert _bwd(n=301, dlogt=F, ws=None, ws_bytes=304) == 1


def test_training_mode_cpu_tensor_still_refused():
    """No CPU fallback on the autograd path either: a training-mode module with a graph wanted reaches the device
    check."""
    disc = ic2.GumbelSoftmaxDiscretization(32, 256).train()
    assert disc.log_temperature.requires_grad
    with pytest.raises(RuntimeError, match="ROCm"):
        disc(torch.zeros(1, 16, 32, requires_grad=True))
    with pytest.raises(RuntimeError, match="ROCm"):
        disc(torch.zeros(1, 16, 32), hard=True)


def test_train_step_gumbel_defaults_are_the_reference_weights():
    """train_gumbel_discretized_hvae's loss weights (gumbel_softmax_compression.py:333-336) and learning rate
    (:328)."""
    p = inspect.signature(ict.train_step_gumbel).parameters
    assert (p["kl_weight"].default, p["perceptual_weight"].default, p["gumbel_weight"].default,
            p["rec_weight"].default) == (0.01, 0.8, 1.0, 1.0)
    assert list(p)[:4] == ["compressor", "images", "optimizer", "w_avg"]
    assert p["percep"].default is None and p["scaler"].default is None
    assert inspect.signature(ict.make_gumbel_optimizer).parameters["lr"].default == 1e-4


def test_train_step_gumbel_refuses_before_touching_the_device():
    """A non-zero perceptual weight without a perceptual loss raises (the reference's LPIPS weights are not
    available), and so does a compressor left in eval mode (the quantizer is inference-only there)."""
    G = ic2.Generator(img_resolution=256)
    enc = ic2.HVAE_VGG_Encoder(img_resolution=64, channel_base=256, channel_max=32, w_dim=512)
    comp = ic2.GumbelSoftmaxCompressor(enc, G)
    opt = ict.make_gumbel_optimizer(comp)
    held = {id(q) for grp in opt.param_groups for q in grp["params"]}
    assert id(comp.discretization.log_temperature) in held and all(id(q) in held for q in enc.parameters())
    assert not any(id(q) in held for q in G.parameters())
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="perceptual"):
        ict.train_step_gumbel(comp, x, opt, torch.zeros(1, 1, 512))
    comp.eval()
    with pytest.raises(RuntimeError, match="training mode"):
        ict.train_step_gumbel(comp, x, opt, torch.zeros(1, 1, 512), perceptual_weight=0.0)
