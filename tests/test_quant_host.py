"""CPU: the refusals of the quantizer entry points (csrc/quant.hip).  Each returns the invalid-argument code before any
launch: the pointers given here are not memory, so a call that went on to launch or write would not return 1."""
import ctypes

import pytest

from image_compression_2_amd import _native as nv

F = ctypes.c_void_p(64)         # a non-null, 16-byte aligned address that is never dereferenced
OK, INVALID = 0, 1


def _uniform(lib, w=F, n=8, bits=8, q=F, idx=F):
    return lib.ic2_quantize_uniform(w, n, bits, q, idx, None)


def _argmin(lib, z=F, n=8, cb=F, k=256, idx=F, zq=F, hist=F):
    return lib.ic2_quantize_codebook_argmin(z, n, cb, k, idx, zq, hist, None)


def _lookup(lib, codes=F, n=8, cb=F, k=256, w=F, oob=F):
    return lib.ic2_codebook_lookup(codes, n, cb, k, w, oob, None)


def _gumbel(lib, z=F, n=8, cb=F, k=256, log_tau=None, tau=0.7, hard=0, noise=F, disc=F, idx=F, psum=F):
    return lib.ic2_gumbel_softmax_quantize(z, n, cb, k, log_tau, tau, hard, 0, 0, noise, disc, idx, psum, None)


def _gumbel_dseed(lib, z=F, n=8, cb=F, k=256, log_tau=None, tau=0.7, hard=0, seed=None, noise=F, disc=F, idx=F,
                  psum=F):
    return lib.ic2_gumbel_softmax_quantize_dseed(z, n, cb, k, log_tau, tau, hard, seed, 0, noise, disc, idx, psum,
                                                 None)


def test_abi_version_is_unchanged():
    assert nv.load().ic2_abi_version() == 1


@pytest.mark.parametrize("bits", [0, 25, -1])
def test_uniform_refuses_bits_outside_1_to_24(bits):
    lib = nv.load()
    assert _uniform(lib, bits=bits) == INVALID
    assert b"bits" in lib.ic2_last_error() and str(bits).encode() in lib.ic2_last_error()


def test_uniform_refuses_sizes_pointers_and_alignment():
    lib = nv.load()
    assert _uniform(lib, n=-1) == INVALID and b"n < 0" in lib.ic2_last_error()
    for kw in ("w", "q"):
        assert _uniform(lib, **{kw: None}) == INVALID and b"null pointer" in lib.ic2_last_error()
    for kw in ("w", "q", "idx"):
        for off in (4, 8, 12):
            assert _uniform(lib, **{kw: ctypes.c_void_p(64 + off)}) == INVALID
            assert b"aligned" in lib.ic2_last_error()


@pytest.mark.parametrize("k", [0, 8193, -3])
def test_argmin_refuses_codebook_sizes(k):
    lib = nv.load()
    assert _argmin(lib, k=k) == INVALID
    assert b"codebook_argmin" in lib.ic2_last_error() and f"k={k}".encode() in lib.ic2_last_error()


def test_argmin_and_lookup_refuse_sizes_and_pointers():
    lib = nv.load()
    assert _argmin(lib, n=-1) == INVALID and b"n=-1" in lib.ic2_last_error()
    for kw in ("z", "cb", "idx"):
        assert _argmin(lib, **{kw: None}) == INVALID and b"null pointer" in lib.ic2_last_error()
    assert _lookup(lib, n=-1) == INVALID and _lookup(lib, k=0) == INVALID
    assert b"codebook_lookup" in lib.ic2_last_error()
    for kw in ("codes", "cb", "w"):
        assert _lookup(lib, **{kw: None}) == INVALID and b"null pointer" in lib.ic2_last_error()


@pytest.mark.parametrize("entry", [_gumbel, _gumbel_dseed], ids=["seed", "dseed"])
def test_gumbel_refusals(entry):
    lib = nv.load()
    for k in (0, 1025, -1):
        assert entry(lib, k=k) == INVALID
        assert b"gumbel_softmax_quantize" in lib.ic2_last_error() and f"k={k}".encode() in lib.ic2_last_error()
    assert entry(lib, n=-1) == INVALID
    for kw in ("z", "cb", "disc"):
        assert entry(lib, **{kw: None}) == INVALID and b"null pointer" in lib.ic2_last_error()
    for tau in (0.0, -0.7, float("nan")):
        assert entry(lib, tau=tau) == INVALID and b"temperature" in lib.ic2_last_error()


def test_gumbel_dseed_needs_a_seed_or_noise():
    lib = nv.load()
    assert _gumbel_dseed(lib, seed=None, noise=None) == INVALID and b"seed_dev" in lib.ic2_last_error()


def test_empty_input_is_ok_for_each_entry():
    lib = nv.load()
    assert _uniform(lib, n=0) == OK and _uniform(lib, n=0, w=None, q=None, idx=None) == OK
    assert _argmin(lib, n=0) == OK and _argmin(lib, n=0, z=None, cb=None, idx=None, zq=None, hist=None) == OK
    assert _lookup(lib, n=0) == OK and _lookup(lib, n=0, codes=None, cb=None, w=None, oob=None) == OK
    assert _gumbel(lib, n=0) == OK and _gumbel(lib, n=0, z=None, cb=None, noise=None, disc=None) == OK
    assert _gumbel_dseed(lib, n=0) == OK and _gumbel_dseed(lib, n=0, noise=None) == OK
