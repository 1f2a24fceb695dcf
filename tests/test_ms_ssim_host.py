"""CPU: the C ABI of the MS-SSIM entry points (ic2_ms_ssim_fwd / ic2_ms_ssim_bwd and their workspace queries): header,
ctypes table and library agree, the queries, and every refusal, which returns before any launch."""
import ctypes
import os
import re

import pytest
import torch

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from image_compression_2_amd import metrics as icm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ic2_ms_ssim_ws_floats", "ic2_ms_ssim_fwd", "ic2_ms_ssim_bwd_ws_floats", "ic2_ms_ssim_bwd"]
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}


def _declarations():
    src = open(os.path.join(ROOT, "include", "ic2ops.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(ic2_ms_ssim\w*)\s*\(([^)]*)\)\s*;", src):
        out[name] = (ret, [a.strip() for a in args.split(",")])
    return out


def test_header_ctypes_table_and_library_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(NAMES)
    lib = nv.load()
    for name, (ret, args) in decl.items():
        assert hasattr(lib, name), name
        expect = [ctypes.c_void_p if "*" in a else _CTYPE[a.rsplit(" ", 1)[0]] for a in args]
        assert nv._SIGS[name] == expect, name
        assert nv._RESTYPE.get(name, ctypes.c_int) is _CTYPE[ret], name
    assert lib.ic2_abi_version() == 1
    # the header names the Python functions each entry point serves
    src = open(os.path.join(ROOT, "include", "ic2ops.h")).read()
    for fn in ("metrics.ms_ssim_terms", "metrics.uint8_ms_ssim", "metrics.ms_ssim", "metrics.ms_ssim_loss"):
        assert fn in src, fn


def test_workspace_queries():
    for q in ("ic2_ms_ssim_ws_floats", "ic2_ms_ssim_bwd_ws_floats"):
        sizes = [nv.query(q, n, 3, 256, 256) for n in (1, 2, 3, 32)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == 4, (q, sizes)
        # 161 and 162 pool to the same 81: monotone, not strictly
        by_side = [nv.query(q, 1, 3, s, s) for s in (161, 162, 163, 200, 256, 1024)]
        assert by_side[0] > 0 and by_side == sorted(by_side) and len(set(by_side)) == 5, (q, by_side)
        assert nv.query(q, 1, 1, 161, 161) < nv.query(q, 1, 2, 161, 161)
        # shapes the entry points refuse need no workspace
        for n, c, h, w in ((1, 3, 160, 256), (1, 3, 256, 160), (0, 3, 256, 256), (1, 0, 256, 256), (1, -1, 256, 256),
                           (1, 3, 0, 0)):
            assert nv.query(q, n, c, h, w) == 0, (q, n, c, h, w)
    # 161 x 161 x 1 plane: the pooled levels 81^2 + 41^2 + 21^2 + 11^2 of both images; forward adds the f64 partials of
    # ceil(151/ty)*ceil(151/tx) + ceil(71/ty)*ceil(71/tx) + 1 + 1 + 1 tiles (two floats each)
    ty, tx = icm.MS_SSIM_TILE
    pyr = 81 * 81 + 41 * 41 + 21 * 21 + 11 * 11
    up = lambda a, b: -(-a // b)
    tiles = sum(up(s - 10, ty) * up(s - 10, tx) for s in (161, 81, 41, 21, 11))
    assert nv.query("ic2_ms_ssim_bwd_ws_floats", 1, 1, 161, 161) == 2 * pyr
    assert nv.query("ic2_ms_ssim_ws_floats", 1, 1, 161, 161) == 2 * pyr + 2 * tiles


def test_refusals_return_before_any_launch():
    lib = nv.load()
    f = ctypes.c_void_p(64)

    def fwd(n=1, c=3, h=161, w=161, mode=0, a=f, b=f, terms=f, ws=f):
        return lib.ic2_ms_ssim_fwd(a, b, mode, n, c, h, w, terms, ws, None)

    def bwd(n=1, c=3, h=161, w=161, mode=0, a=f, b=f, ws_fwd=f, gterms=f, ga=f, gb=f, ws_grad=f):
        return lib.ic2_ms_ssim_bwd(a, b, mode, ws_fwd, gterms, n, c, h, w, ga, gb, ws_grad, None)

    for call in (fwd, bwd):
        for h, w in ((160, 161), (161, 160), (100, 300), (11, 11)):
            assert call(h=h, w=w) == 1
            assert b"160" in lib.ic2_last_error() and f"h={h} w={w}".encode() in lib.ic2_last_error()
        for kw in (dict(c=0), dict(c=-2), dict(n=0), dict(h=0), dict(w=-5)):
            assert call(**kw) == 1
            assert b"positive" in lib.ic2_last_error()
        assert call(mode=7) == 1 and b"mode=7" in lib.ic2_last_error()
    for kw in ("a", "b", "terms", "ws"):
        assert fwd(**{kw: None}) == 1 and b"null pointer" in lib.ic2_last_error()
    assert fwd(ws=ctypes.c_void_p(68)) == 1 and b"aligned" in lib.ic2_last_error()
    for kw in ("a", "b", "ws_fwd", "gterms", "ws_grad"):
        assert bwd(**{kw: None}) == 1 and b"null pointer" in lib.ic2_last_error()
    assert bwd(ga=None, gb=None) == 1 and b"null pointer" in lib.ic2_last_error()
    # the metric has no backward: IC2_E_UNSUPPORTED, whatever else the call says
    assert bwd(mode=1) == 2 and b"metric" in lib.ic2_last_error()


def test_python_layer_refuses_cpu_tensors_and_small_images():
    x = torch.zeros(1, 3, 161, 161)
    for fn in (ic2.ms_ssim_terms, ic2.uint8_ms_ssim, ic2.ms_ssim, ic2.ms_ssim_loss, ic2.MSSSIMLoss()):
        with pytest.raises(RuntimeError, match="ROCm"):
            fn(x, x)
    assert ic2.MS_SSIM_TILE == icm.MS_SSIM_TILE and len(list(ic2.MSSSIMLoss().parameters())) == 0
    import ms_ssim_oracle as mo
    assert icm.MS_SSIM_TILE == mo.TILE      # the oracle's case table derives its tile shapes from a literal
    assert icm.MS_SSIM_WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def test_training_docstring_names_the_offline_perceptual_term():
    from image_compression_2_amd import training as ict
    assert "metrics.MSSSIMLoss()" in ict.__doc__
    with pytest.raises(ValueError, match="perceptual_weight != 0 needs a perceptual loss callable"):
        ict.train_step(None, None, None, None)      # percep=None with the default weight 0.8 still raises, first thing
