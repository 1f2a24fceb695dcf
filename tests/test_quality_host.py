"""CPU: the SSIM restatement the GPU tests compare against, the argument validation of ic2_uint8_quality, and the
host arithmetic that turns (all-reduced) sums into the evaluation record's figures."""
import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from image_compression_2_amd import distributed as icd
from image_compression_2_amd import metrics as icm

import ssim_oracle as so

# the shapes tests/test_gpu_quality.py compares the kernel at (its two tile-derived shapes included)
_OY, _OX = icm.QUALITY_TILE
SHAPES = [(2, 3, 7, 7), (2, 3, 8, 11), (1, 1, 7, 64), (1, 3, 23, 70), (3, 3, 33, 65), (1, 3, 64, 64), (1, 3, 256, 256),
          (1, 3, _OY + 5, _OX + 5), (1, 3, _OY + 7, _OX + 7)]


def _pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2.4 - 1.2, torch.rand(shape, generator=g) * 2 - 1


# ------------------------------------------------------------------ the restatement, pinned three ways
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_bruteforce_integer_moments(shape):
    """uniform_filter + crop against exact integer moments of every fully-inside window: the two formulations differ
    by float64 rounding only (observed <= 8e-16 over these shapes)."""
    from oracle import metrics as om
    a, b = _pair(shape)
    noisy = a + 0.05 * torch.randn(shape, generator=torch.Generator().manual_seed(1))
    for x, y in ((a, b), (a, noisy)):
        ux, uy = om.to_uint8(x), om.to_uint8(y)
        for i in range(shape[0]):
            wins = [7] + ([3, 11] if 11 <= min(shape[2:]) <= 64 else [])
            for win in wins:
                got, ref = so.ssim_uint8(ux[i], uy[i], win), so.ssim_bruteforce(ux[i], uy[i], win)
                assert abs(got - ref) <= 1e-12, (shape, i, win, got, ref)


def test_restatement_identical_images_give_exactly_one():
    a, _ = _pair((2, 3, 23, 70))
    assert so.ssim_batch(a, a).tolist() == [1.0, 1.0]


@pytest.mark.parametrize("u,v,expect", [(255, 0, 9.9990001e-5), (165, 167, 0.99992743172), (0, 0, 1.0)])
def test_restatement_constant_images_closed_form(u, v, expect):
    """Constant images have zero variances: S = (2uv + C1) / (u^2 + v^2 + C1) in every window."""
    x = np.full((16, 19, 3), u, np.uint8)
    y = np.full((16, 19, 3), v, np.uint8)
    closed = (2 * u * v + so.C1) / (u * u + v * v + so.C1)
    # the filter's running sums leave the variances at a few ulp(255^2) = 7e-12 instead of 0: over C2 = 58.5, < 1e-12
    assert so.ssim_uint8(x, y) == pytest.approx(closed, abs=1e-12)
    assert closed == pytest.approx(expect, rel=1e-8)


def test_restatement_refuses_what_skimage_refuses():
    x = np.zeros((6, 9, 3), np.uint8)
    with pytest.raises(ValueError):
        so.ssim_uint8(x, x)
    with pytest.raises(ValueError):
        so.ssim_uint8(np.zeros((9, 9, 3), np.uint8), np.zeros((9, 9, 3), np.uint8), win_size=4)


# ------------------------------------------------------------------ the entry point validates before any launch
def test_uint8_quality_argument_errors_are_reported_without_a_gpu():
    lib = nv.load()
    f = ctypes.c_void_p(16)

    def call(n, c, h, w, win, a=f, b=f, sse=f, ssim=f, scratch=f):
        return lib.ic2_uint8_quality(a, b, n, c, h, w, win, sse, ssim, scratch, None)

    assert call(1, 3, 16, 16, 4) == 1
    assert b"win=4" in lib.ic2_last_error()
    assert call(1, 3, 16, 16, 13) == 1
    assert b"win=13" in lib.ic2_last_error()
    assert call(1, 3, 6, 16, 7) == 1
    assert b"win=7" in lib.ic2_last_error() and b"h=6" in lib.ic2_last_error()
    assert call(1, 3, 16, 5, 7) == 1
    assert b"win=7" in lib.ic2_last_error() and b"w=5" in lib.ic2_last_error()
    for kw in ("a", "b", "sse", "ssim", "scratch"):
        assert call(1, 3, 16, 16, 7, **{kw: None}) == 1
        assert b"null pointer" in lib.ic2_last_error()
    for n, c, h, w in ((0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 0, 16), (1, 3, 16, -1)):
        assert call(n, c, h, w, 7) == 1
        assert b"positive" in lib.ic2_last_error()


def test_uint8_quality_scratch_query():
    q = lambda *a: nv.query("ic2_uint8_quality_scratch_doubles", *a)
    sizes = [q(n, 3, 256, 256, 7) for n in (1, 2, 3, 32)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == 4
    # two partials (SSIM sum, squared error) per tile of QUALITY_TILE window origins per (image, channel)
    oy, ox = icm.QUALITY_TILE
    assert q(2, 3, 256, 256, 7) == 2 * 2 * 3 * math.ceil(250 / oy) * math.ceil(250 / ox)
    assert q(1, 1, 7, 7, 7) == 2
    # shapes the entry point refuses need no scratch
    assert q(1, 3, 6, 16, 7) == 0 and q(1, 3, 16, 16, 4) == 0 and q(0, 3, 16, 16, 7) == 0


def test_product_path_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="ROCm"):
        ic2.uint8_quality(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


# ------------------------------------------------------------------ sums -> figures
def test_ssim_from_sums():
    assert ic2.ssim_from_sums(12.5, 50) == 0.25
    assert icm.ssim_from_sums(torch.tensor(3.0, dtype=torch.float64), 3) == 1.0
    assert icm.n_windows(23, 70, 7) == 17 * 64 and icm.n_windows(7, 7) == 1


def test_figures_from_hand_made_sums():
    # 2 images of 3 x 8 x 8 (4 windows each per channel): MSE 4 without, 16 with quantization
    n_values, n_win = 2 * 3 * 64, 2 * 3 * 4
    vec = icm.quality_record(4.0 * n_values, 0.75 * n_win, 16.0 * n_values, 0.5 * n_win, n_values, n_win, 2)
    assert vec.dtype == torch.float64 and vec.numel() == 7
    fig = icm.figures_from_record(vec)
    assert fig == {"n_images": 2,
                   "batch_psnr_no_quant": 10 * math.log10(255.0 ** 2 / 4.0),
                   "batch_ssim_no_quant": 0.75,
                   "batch_psnr_quantized": 10 * math.log10(255.0 ** 2 / 16.0),
                   "batch_ssim_quantized": 0.5}
    zero = icm.figures_from_record(icm.quality_record(0.0, n_win, 0.0, n_win, n_values, n_win, 2))
    assert zero["batch_psnr_quantized"] == float("inf") and zero["batch_ssim_quantized"] == 1.0


def _synthetic_sums(n):
    """Per-image sums as ic2_uint8_quality would give them for n images of 3 x 16 x 16 (squared errors are integers)."""
    g = torch.Generator().manual_seed(5)
    sse_nq = torch.randint(0, 10 ** 6, (n,), generator=g).double()
    sse_q = torch.randint(0, 10 ** 6, (n,), generator=g).double()
    ssim_nq = torch.rand(n, 3, generator=g, dtype=torch.float64) * 100
    ssim_q = torch.rand(n, 3, generator=g, dtype=torch.float64) * 100
    return sse_nq, ssim_nq, sse_q, ssim_q


def _record(sums, lo, hi):
    sse_nq, ssim_nq, sse_q, ssim_q = (t[lo:hi] for t in sums)
    n = hi - lo
    return icm.quality_record(sse_nq.sum().item(), ssim_nq.sum().item(), sse_q.sum().item(), ssim_q.sum().item(),
                              n * 3 * 256, n * 3 * 100, n)


def _worker(rank, world, port, n, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    icd.init(backend="gloo")
    s, e = icd.shard(n, rank, world)
    vec = icd.allreduce_sum(_record(_synthetic_sums(n), s, e))
    icd.barrier()
    if rank == 0:
        out_q.put(vec.numpy())
    dist.destroy_process_group()


def test_reduced_figures_equal_single_process_figures_world2():
    """Each rank contributes the sums of its own shard; the figures formed from the all-reduced record equal those of
    the whole batch in one process (the SSIM sums up to the rounding of one reordered float64 addition)."""
    world, n = 2, 5
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    vec = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    whole = _record(_synthetic_sums(n), 0, n)
    assert np.array_equal(vec[[0, 1, 2, 4, 5]], whole.numpy()[[0, 1, 2, 4, 5]])   # integers: exact
    got, ref = icm.figures_from_record(vec), icm.figures_from_record(whole)
    assert got["n_images"] == ref["n_images"] == n
    for k in ("batch_psnr_no_quant", "batch_psnr_quantized"):
        assert got[k] == ref[k]
    for k in ("batch_ssim_no_quant", "batch_ssim_quantized"):
        assert got[k] == pytest.approx(ref[k], rel=1e-14, abs=0)
