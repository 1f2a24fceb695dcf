"""CPU: the fp64 MS-SSIM restatement (tests/ms_ssim_oracle.py) pinned without the library, and the conditions its case
table rests on."""
import numpy as np
import pytest
import torch

import ms_ssim_oracle as mo


def _img(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_identical_images_give_terms_exactly_one():
    x = _img((2, 3, 163, 189), 0)
    terms = mo.terms_of(x, x.clone(), 1.0)
    assert terms.shape == (2, 3, 5) and terms.tolist() == [[[1.0] * 5] * 3] * 2
    assert mo.value_of(terms).tolist() == [1.0, 1.0]
    u = mo.to_uint8(x * 2 - 1)
    assert mo.terms_of(u, u.clone(), 255.0).tolist() == [[[1.0] * 5] * 3] * 2


@pytest.mark.parametrize("p,q", [(0.25, 0.75), (0.9, 0.1), (0.5, 0.5)])
def test_constant_images_closed_form(p, q):
    """Zero variances: cs = 1 at every scale (the pool's zero border is shared by both images, so sigma_xy tracks
    sigma_x sigma_y only inside; a constant image stays constant where no padding enters), value = luminance^0.1333."""
    shape = (1, 2, 176, 192)     # every level even: 176 -> 88 -> 44 -> 22 -> 11, 192 -> 96 -> 48 -> 24 -> 12
    x, y = torch.full(shape, p, dtype=torch.float64), torch.full(shape, q, dtype=torch.float64)
    terms = mo.terms_of(x, y, 1.0)
    assert (terms[..., :4] - 1.0).abs().max().item() <= 1e-12
    c1 = 0.01 ** 2
    lum = (2 * p * q + c1) / (p * p + q * q + c1)
    assert terms[..., 4].numpy() == pytest.approx(lum, abs=1e-12)
    assert mo.value_of(terms).numpy() == pytest.approx(lum ** 0.1333, abs=1e-12)


def test_data_range_scaling_invariance():
    a, b = mo.inputs((1, 3, 163, 189), "noisy")
    ua, ub = mo.to_uint8(a), mo.to_uint8(b)
    t255 = mo.terms_of(ua, ub, 255.0)
    t1 = mo.terms_of(ua / 255.0, ub / 255.0, 1.0)
    assert (t255 - t1).abs().max().item() <= 1e-12


def test_pool_pads_odd_axes_at_both_ends():
    x = _img((1, 1, 161, 189), 3)
    p = mo.pool(x)
    assert p.shape == (1, 1, 81, 95)
    assert p[0, 0, 0, 0].item() == x[0, 0, 0, 0].item() / 4
    assert p[0, 0, 1, 1].item() == pytest.approx(x[0, 0, 1:3, 1:3].mean().item(), abs=1e-15)
    assert p[0, 0, 80, 94].item() == pytest.approx(x[0, 0, 159:161, 187:189].mean().item(), abs=1e-15)
    e = _img((1, 1, 162, 188), 4)
    assert torch.equal(mo.pool(e), torch.nn.functional.avg_pool2d(e, 2))
    # the adjoint is the adjoint: <pool x, g> == <x, pool_t g>
    g = _img((1, 1, 81, 95), 5)
    assert (mo.pool(x) * g).sum().item() == pytest.approx((x * mo.pool_t(g, 161, 189)).sum().item(), rel=1e-13)


def test_transposed_filter_is_the_adjoint():
    x, g = _img((1, 1, 30, 41), 6), _img((1, 1, 20, 31), 7)
    assert (mo.gfilt(x) * g).sum().item() == pytest.approx((x * mo.gfilt_t(g)).sum().item(), rel=1e-13)


def test_scale_zero_equals_direct_window_evaluation():
    """Scale 0 of one 161 x 161 plane against sums over explicit 11 x 11 windows (no convolution)."""
    a, b = mo.inputs((2, 3, 161, 161), "smooth")
    x, y = mo.loss_images(a)[0, 0].numpy(), mo.loss_images(b)[0, 0].numpy()
    g = mo.window().numpy()
    w2 = np.outer(g, g)
    assert abs(w2.sum() - 1.0) <= 1e-15
    vx = np.lib.stride_tricks.sliding_window_view(x, (11, 11))
    vy = np.lib.stride_tricks.sliding_window_view(y, (11, 11))
    assert vx.shape == (151, 151, 11, 11)
    mx, my = (vx * w2).sum((2, 3)), (vy * w2).sum((2, 3))
    sxx = (vx * vx * w2).sum((2, 3)) - mx * mx
    syy = (vy * vy * w2).sum((2, 3)) - my * my
    sxy = (vx * vy * w2).sum((2, 3)) - mx * my
    c2 = 0.03 ** 2
    direct = ((2 * sxy + c2) / (sxx + syy + c2)).mean()
    got = mo.loss_terms(a, b)[0, 0, 0].item()
    assert abs(got - direct) <= 1e-13


def test_small_images_are_refused():
    x = torch.zeros(1, 1, 160, 200, dtype=torch.float64)
    with pytest.raises(ValueError):
        mo.terms_of(x, x, 1.0)


def test_zero_gradient_convention():
    """A channel with a term <= 0 has value 0 and gradient 0; the other channels and images keep theirs."""
    terms = torch.tensor([[[0.9, 0.8, -0.1, 0.7, 0.6], [0.9, 0.8, 0.5, 0.7, 0.6]]], dtype=torch.float64)
    g = mo.gterms_of(terms, torch.tensor([2.0], dtype=torch.float64))
    assert g[0, 0].tolist() == [0.0] * 5 and torch.isfinite(g).all()
    w = torch.tensor(mo.WEIGHTS, dtype=torch.float64)
    v1 = (terms[0, 1] ** w).prod()
    assert g[0, 1].numpy() == pytest.approx((-2.0 / 2 * w * v1 / terms[0, 1]).numpy(), rel=1e-13)


@pytest.mark.parametrize("kind", ["noisy", "smooth"])
def test_case_table_value_cases_are_well_conditioned(kind):
    """The value and gradient bars of tests/test_gpu_ms_ssim.py rest on every reference term of these cases staying
    above 0.5 (max(t, 0)^w is then smooth), in both modes and at every shape of the table."""
    for shape in mo.SHAPES + mo.tile_shapes():
        for mode in ("loss", "metric"):
            assert mo.reference(shape, kind, mode)["terms"].min().item() > 0.5, (shape, mode)


def test_case_table_negated_has_value_zero_and_independent_starts_near_zero():
    neg = mo.reference((1, 3, 163, 189), "negated", "loss")
    assert neg["terms"].min().item() < -0.5 and neg["value"].tolist() == [0.0]
    ind = mo.reference((1, 3, 163, 189), "independent", "loss")
    # scale 0 sits next to zero, where max(t, 0)^0.0448 amplifies without bound: the GPU tests compare its terms only
    assert ind["terms"][..., 0].abs().max().item() < 0.05


def test_gradient_of_negated_is_zero_and_bound_is_zero():
    r = mo.reference_grads((1, 1, 161, 200), "negated")
    assert not r["ga"].any() and not r["gb"].any() and not r["Ga"].any()
