"""CPU: pin tests/quant_oracle.py without the native library: against oracle/encoder.py (itself pinned to the
reference's outputs), against the reference's golden vectors, on a hand-written codebook for the tie rule, and on
non-finite latents."""
import os

import numpy as np
import pytest
import torch

import quant_oracle as qo
from oracle import encoder as oe


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


@pytest.mark.parametrize("bits", [1, 2, 4, 8, 10, 16, 24])
def test_uniform_is_the_encoder_oracle(bits):
    w = torch.rand(5000, generator=torch.Generator().manual_seed(bits)) * 3 - 1.5
    q, idx = qo.uniform(w, bits)
    assert torch.equal(q, oe.quantize_uniform(w, bits))
    assert torch.equal(idx, oe.uniform_indices(w, bits))
    assert q.dtype == torch.float32 and idx.dtype == torch.int64


@pytest.mark.parametrize("bits", [4, 8, 10])
@pytest.mark.parametrize("tag", ["rand", "adv"])
def test_uniform_matches_reference_golden(golden_dir, bits, tag):
    d = _load(golden_dir, "quantizers.npz")
    q, _ = qo.uniform(torch.from_numpy(d[f"uniform_b{bits}_{tag}_w"]), bits)
    assert torch.equal(q, torch.from_numpy(d[f"uniform_b{bits}_{tag}_q"]))


@pytest.mark.parametrize("bits", [1, 2, 7, 8, 12, 16, 23, 24])
def test_uniform_grid_requantizes_and_halfway_points_are_halfway(bits):
    s = (1 << bits) - 1
    w, r = qo.uniform_grid(bits, count=100000 if bits > 16 else None)
    q, idx = qo.uniform(w, bits)
    assert torch.equal(idx, r) and torch.equal(q, w)
    assert r.min().item() == 0 or bits > 16
    wh, rh = qo.uniform_halfway(bits)
    assert wh.numel() > 0
    prod = ((wh + 1.0) * 0.5) * float(s)
    assert torch.equal(prod.double(), rh.double() + 0.5)        # exactly half-way in f32
    _, ih = qo.uniform(wh, bits)
    assert torch.equal(ih, rh + (rh % 2))                       # half to even
    assert bool((rh % 2 == 0).any()) and (bits == 1 or bool((rh % 2 == 1).any()))


def test_argmin_is_the_encoder_oracle_and_the_golden(golden_dir):
    d = _load(golden_dir, "quantizers.npz")
    z = torch.from_numpy(d["codebook_z"])
    cb = torch.from_numpy(d["codebook"])
    idx = qo.argmin(z, cb)
    assert torch.equal(idx, oe.codebook_argmin(z)) and np.array_equal(idx.numpy(), d["codebook_idx"])
    # chunking changes nothing
    old = qo.ARGMIN_CHUNK
    try:
        qo.ARGMIN_CHUNK = 256 * 1000
        assert torch.equal(qo.argmin(z, cb), idx)
    finally:
        qo.ARGMIN_CHUNK = old


def test_tie_rule_on_a_codebook_with_a_duplicate():
    cb = torch.tensor([0.5, -0.25, 0.5, 1.0, -1.0])
    z = torch.tensor([0.5, 0.4, 0.75, 0.125, -0.625, -2.0, 2.0, 0.6])
    #   0.5: entries 0 and 2 tie at distance 0 -> 0;  0.75: 0.5 (0, 2) and 1.0 (3) tie at 0.25 -> 0
    #   0.125: -0.25 (1) and 0.5 (0, 2) tie at 0.375 -> 0;  -0.625: -0.25 (1) and -1.0 (4) tie -> 1
    assert qo.argmin(z, cb).tolist() == [0, 0, 0, 0, 1, 4, 3, 0]
    w, oob = qo.lookup(torch.tensor([0, 4, 2]), cb)
    assert w.tolist() == [0.5, -1.0, 0.5] and oob is False
    w, oob = qo.lookup(torch.tensor([5, -1, 3, 2 ** 32]), cb)
    assert w.tolist() == [0.0, 0.0, 1.0, 0.0] and oob is True
    # the Gumbel reference's top-1 takes the first index among equal y as well
    noise = torch.zeros(1, 5)
    r = qo.gumbel(torch.tensor([0.5]), cb, noise, 1.0, True)
    assert r["top1"].tolist() == [0] and r["top2"].tolist() == [2] and r["gap"].tolist() == [0.0]
    assert r["idx"].tolist() == [0] and bool(r["ambiguous"][0])


def test_non_finite_latents_give_index_zero():
    cb = torch.linspace(-1, 1, 7)
    z = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.9])
    assert qo.argmin(z, cb).tolist() == [0, 0, 0, 6]
    assert torch.argmin(torch.abs(z.reshape(-1, 1) - cb.reshape(1, -1)), dim=1).tolist() == [0, 0, 0, 6]
    r = qo.gumbel(z, cb, torch.zeros(4, 7), 0.7, False)
    assert r["idx"].tolist() == [0, 0, 0, 6]
    assert bool(r["disc"][:3].isnan().all()) and bool(r["disc"][3].isfinite())
    assert bool(r["psum"].isnan().all())


@pytest.mark.parametrize("k,tau,hard", [(256, 0.7, False), (256, 0.7, True), (100, 0.1, False), (1000, 5.0, True),
                                        (1, 1.0, False), (2, 1.0, True)])
def test_gumbel_is_the_encoder_oracle(k, tau, hard):
    """The fp64 reference against oracle/encoder.py's f32 composition, within the bound the kernel is held to (torch's
    f32 softmax and matmul make no more roundings than the count of the docstring)."""
    n = 257
    g = torch.Generator().manual_seed(k)
    z = torch.rand(n, generator=g) * 2.4 - 1.2
    noise = oe.gumbel_noise(k + 1, n, k)
    cb = oe.codebook(k) if k > 1 else torch.tensor([-1.0])
    r = qo.gumbel(z, cb, noise, tau, hard)
    if k > 1:
        disc, perp, idx = oe.gumbel_forward(z, noise, tau, hard, n_embeddings=k)
        assert torch.equal(idx, r["idx"])
        clear = ~r["ambiguous"]
        assert clear.float().mean().item() > 0.99
        err = (disc.double() - r["disc"]).abs()
        assert bool((err[clear] <= r["disc_bound"](qo.K_DISC_DERIVED)[clear]).all())
        avg = r["psum"] / n
        ref_perp = torch.exp(-torch.sum(avg * torch.log(avg + 1e-10))).item()
        if bool(clear.all()):
            assert abs(perp.item() - ref_perp) <= 1e-5 * ref_perp
    assert abs(r["psum"].sum().item() - n) <= 1e-9 * n
    assert r["terms"] == 1 + 3 + 65 and qo.gumbel_terms(16389) == 2 + 3 + 4096 and qo.gumbel_terms(1) == 5
    assert bool((r["W"] >= r["Y"]).all()) and bool((r["W"] >= r["D"]).all())


@pytest.mark.parametrize("case", range(4))
def test_gumbel_matches_reference_golden(golden_dir, case):
    d = _load(golden_dir, "gumbel_forward.npz")
    _, tau, hard, _ = d[f"c{case}_meta"]
    z = torch.from_numpy(d["z"])
    noise = torch.from_numpy(d["noise"])
    tau32 = torch.exp(torch.ones(1) * np.log(tau)).item()       # the module's temperature, an f32
    r = qo.gumbel(z, oe.codebook(256), noise, tau32, bool(hard))
    assert torch.equal(r["idx"], torch.from_numpy(d[f"c{case}_idx"]))
    disc = torch.from_numpy(d[f"c{case}_disc"]).reshape(-1).double()
    clear = ~r["ambiguous"]
    assert bool(clear.all())
    if hard:
        assert torch.equal(disc, r["disc"])
    else:
        assert bool(((disc - r["disc"]).abs() <= r["disc_bound"](qo.K_DISC_DERIVED)).all())
    avg = r["psum"] / z.numel()
    ref_perp = torch.exp(-torch.sum(avg * torch.log(avg + 1e-10))).item()
    assert abs(float(d[f"c{case}_perplexity"]) - ref_perp) <= 1e-5 * ref_perp


def test_codebook_builders():
    for k in (255, 256, 1024):
        cb = qo.codebook_shuffled(k, seed=k)
        assert cb.numel() == k and torch.unique(cb).numel() == k - 3
        assert qo.midpoints(cb).numel() == k - 1
    assert qo.midpoints(torch.tensor([0.25])).numel() == 0
