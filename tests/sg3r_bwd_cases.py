"""TEST INFRASTRUCTURE -- geometries, filters and stored operands of the radial (2-D down filter) filtered-lrelu
backward cases, shared by tests/test_sg3r_bwd_host.py (which pins them on the CPU) and tests/test_gpu_sg3r_train.py.

Built on tests/flrelu_bwd_oracle.py (``reference`` accepts a 2-D ``fd``: oracle/sg3.py's upfirdn2d / filtered_lrelu
compute 2-D filters) and tests/sg3r_oracle.py (the radial design).  References are cached per case: the GPU tests
that share a case compute it once and must leave it unchanged.
"""
import numpy as np
import torch

import flrelu_bwd_oracle as fo
import sg3r_oracle as so
from oracle import sg3

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
N, C, C_P = 2, 22, 32
# (x, gout, gx) dtypes of ic2_flrelu_bwd_nhwc_2d's instances
TRIPLES = [(F32, F32, F32), (F16, BF16, BF16), (F16, F16, F16), (F16, F32, F32)]
# the gx tile per up factor (rows, columns): one ydot partial per tile (csrc/flrelu_radial_bwd.hip RbTile)
TILE = {2: (16, 16), 4: (8, 16)}
# the kernel recomputes U in f32 from the stored x in every instance and keeps U, gV and gU as f32 in LDS, so the
# mask allowance A is taken at the f32 unit; the host test asserts the 20 % cap at 2^-11, which contains it (the
# fragile set grows with eps_x)
EPS_X = 2.0 ** -24
EPS_X_HOST = 2.0 ** -11

# paddings: the R layers' and the other gout phase (px0 one less: the polyphase offset R of the kernel flips)
PADS = {2: {"r": [11, 10, 11, 10], "ph": [10, 11, 10, 11]}, 4: {"r": [-2, -5, -2, -5], "ph": [-1, -6, -1, -6]}}
# (in_h, in_w).  Up 2, 16 x 16 tiles: one partial tile, one short of / equal to / one past a tile (15, 16, 17), two
# tiles +- 1 (31, 33).  Up 4, 8 x 16 tiles: rows 13 (8 + 5), 15 / 16 / 17 (one short of, equal to, one past two
# tiles), 24 / 25 (three tiles, one past), 33; columns 15 / 16 / 17 and 21
SIZES = {2: [(5, 7), (16, 15), (17, 33), (31, 17), (15, 16)], 4: [(13, 15), (15, 17), (16, 21), (33, 21), (24, 16), (25, 17)]}


def geometries(which=("r", "ph")):
    """[(id, up, padding, in_h, in_w)]"""
    out = []
    for up in (2, 4):
        for key in which:
            for h, w in SIZES[up]:
                out.append((f"u{up}-{key}-{h}x{w}", up, PADS[up][key], h, w))
    return out


def out_size(in_h, in_w, up, padding):
    return sg3.filtered_lrelu_out_size(in_h, in_w, 6 * up, 12, up, 2, padding)


def nonsym_filters(up, seed=3):
    """(fu [6 up], fd [12, 12]) float32 tensors: a non-symmetric separable up filter and a non-symmetric full-rank
    down filter with unit DC gain (the construction of test_gpu_sg3r._nonsym_filters, restated): the real filters are
    symmetric and would hide a transposed or unflipped tap table."""
    rng = np.random.default_rng(seed)
    fu = sg3.design_lowpass_filter(6 * up, 8.0, 4.0, 64).numpy().astype(np.float64) * (1 + 0.4 * rng.random(6 * up))
    fd = rng.standard_normal((12, 12)) * 0.3 + np.outer(np.hanning(14)[1:-1], np.hanning(14)[1:-1])
    fd /= fd.sum()
    assert not np.allclose(fd, fd.T) and not np.allclose(fd, fd[::-1, ::-1])
    return (torch.from_numpy(np.ascontiguousarray(fu / fu.sum(), np.float32)),
            torch.from_numpy(np.ascontiguousarray(fd, np.float32)))


R256_LAYER = {2: "L0_36_1024", 4: "L3_52_1024"}
_r256 = {}


def r256_filters(up):
    """(fu, fd [12, 12]) float32 tensors of the real R-256 layer L0_36_1024 (up 2) / L3_52_1024 (up 4)."""
    if not _r256:
        _, table = sg3.layer_table(256, **so.R_TABLE_KW)
        _r256.update({L["name"]: L for L in table})
    L = _r256[R256_LAYER[up]]
    assert L["up"] == up and L["padding"] == PADS[up]["r"] and L["down_taps"] == 12
    return (L["up_filter"].float().contiguous(),
            torch.from_numpy(np.ascontiguousarray(so.layer_design(L), np.float32)))


def filters(up, which):
    return nonsym_filters(up) if which == "nonsym" else r256_filters(up)


def _seed(gid):
    return 7 + sum(ord(ch) * (i + 1) for i, ch in enumerate(gid)) % 100000


def case_inputs(gid, up, padding, in_h, in_w, tier, xdt=F32, gdt=F32, gscale=1.0):
    """The stored operands of one case: x (xdt), gout (gdt), oscale, bias.  Linear tier: Gaussian x (no mask decision
    exists); mask tier: block-sign x (flrelu_bwd_oracle.MASK_INPUT)."""
    seed = _seed(gid)
    oh, ow = out_size(in_h, in_w, up, padding)
    if tier == "mask":
        x = fo.block_sign_input(N, in_h, in_w, C, C_P, seed, xdt, *fo.MASK_INPUT[up])
    else:
        x = fo.gauss(N, in_h, in_w, C, C_P, seed, xdt, 3.0)
    gout = fo.gauss(N, oh, ow, C, C_P, seed + 1, gdt, gscale)
    os_, b = fo.scale_bias(N, C, C_P, seed + 2)
    return x, gout, os_, b


_refs = {}


def reference(key, x, gout, fu, fd, up, padding, tier, flip, oscale, bias, eps_x=EPS_X):
    """fo.reference of the case, cached under `key` (None: not cached)."""
    if key is not None and key in _refs:
        return _refs[key]
    r = fo.reference(x, gout, fu, fd, up, padding, flip=bool(flip), oscale=oscale, bias=bias, eps_x=eps_x, c=C,
                     **fo.TIERS[tier])
    if key is not None:
        _refs[key] = r
    return r


def adjoint2d_bruteforce(gout, fd, flip, nky, nkx):
    """One plane: gV[ky][kx] = sum_{oy, ox} gd2[ky - 2 oy][kx - 2 ox] gout[oy][ox] on an nky x nkx grid, as loops, with
    gd2 = fd flipped in both axes unless `flip` (upfirdn2d correlates with the flipped filter; row = y)."""
    t = fd.shape[0]
    gd2 = [[float(fd[a][b]) if flip else float(fd[t - 1 - a][t - 1 - b]) for b in range(t)] for a in range(t)]
    oh, ow = gout.shape
    out = [[0.0] * nkx for _ in range(nky)]
    for ky in range(nky):
        for kx in range(nkx):
            s = 0.0
            for oy in range(max(0, (ky - t + 2) // 2), min(oh, ky // 2 + 1)):
                for ox in range(max(0, (kx - t + 2) // 2), min(ow, kx // 2 + 1)):
                    s += gd2[ky - 2 * oy][kx - 2 * ox] * float(gout[oy, ox])
            out[ky][kx] = s
    return out


def linear_backward_bruteforce(gout, fu, fd, up, padding, gain, flip, in_h, in_w):
    """One plane of the backward with slope 1 and no clamp, as loops: gx[i][j] = sum_{k, l} g_u[i up + py0 - k]
    g_u[j up + px0 - l] gain gV[k][l], g_u[t] = fu[tu - 1 - t] up (fu[t] up when `flip`), gV the 2-D adjoint above."""
    px0, px1, py0, py1 = padding
    tu = fu.shape[0]
    nky, nkx = in_h * up + py0 + py1 - (tu - 1), in_w * up + px0 + px1 - (tu - 1)
    gv = adjoint2d_bruteforce(gout, fd, flip, nky, nkx)
    gu = [float(fu[t] if flip else fu[tu - 1 - t]) * up for t in range(tu)]
    out = torch.zeros(in_h, in_w, dtype=torch.float64)
    for i in range(in_h):
        for j in range(in_w):
            s = 0.0
            for k in range(max(0, i * up + py0 - tu + 1), min(nky, i * up + py0 + 1)):
                for l in range(max(0, j * up + px0 - tu + 1), min(nkx, j * up + px0 + 1)):
                    s += gu[i * up + py0 - k] * gu[j * up + px0 - l] * gv[k][l]
            out[i, j] = s * gain
    return out
