"""TEST INFRASTRUCTURE -- lattice operands, fp64 reference and case table that pin every conv launch-plan instance
bit for bit (tests/test_conv_lattice_host.py on the CPU, tests/test_gpu_conv_lattice.py on the GPU).

Why a lattice.  With small-integer operands every product and every partial sum of a convolution is an integer that
f32 represents exactly, in ANY summation order: the MFMA's internal tree, the K-chunk ring, split-K partials added in
slice order, the two halves of a split tail, Winograd's transforms.  An instance that is correct therefore reproduces
the fp64 convolution bit for bit, and one dropped, duplicated or mis-addressed K element changes an integer.

Operands (seeded per row, exact in f32, bf16 and f16):
  x  integers in [-4, 4], NHWC [n][h][w][cin_p], channels >= cin zero;
  w  direct kernels: integers in [-2, 2], [cout_p][kh][kw][cin_p], rows >= cout_valid and channels >= cin zero;
     Winograd: the same layout with EVEN integers in [-4, 4]; the kernel's operand is U = G w, packed by
     ic2_pack_weight_wino (prenorm 0, scale 1) from the OIHW view of the same tensor.

Exactness conditions (asserted per row by the host test):
  direct    |x w| <= 8, so every partial sum of the K = kh kw cin_p products is an integer of magnitude <= 8 K
            <= 73 728 for K <= 9 * 1024;
  Winograd  G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1] on even |w| <= 4 gives integers |U| <= 6 (three halves of even
            numbers); B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1] on |x| <= 4 gives integers |V| <= 8; both are exact
            in f16.  |U V| <= 48 and a transformed accumulator sums 3 cin_p of them: <= 48 * 3 * cin_p <= 147 456 for
            cin_p <= 1024.  The output transform A^T adds three accumulators: <= 442 368.
  All of these are below 2^24, so f32 holds every intermediate exactly.

Epilogues (ic2ops.h: v = acc * oscale[n][o] + bias[o]; act: v = clamp(lrelu(v) * gain); y = v * out_mul).  Every
constant is a power of two or a small dyadic number, so each f32 operation is exact (the result needs < 24 bits: the
host test asserts that the fp64 value survives a round trip through f32), with or without FMA contraction:
  none    oscale = NULL, bias = NULL, no activation;
  linear  oscale[n][o] = 2^-e, e per (n, o) from {0..3}; bias[o] = k / 8, k in [-16, 16]; out_mul 1.  Values carry
          three fractional bits below an integer part of up to ~12 bits: more than the 11 (f16) / 8 (bf16) significant
          bits of the 16-bit outputs, so their round-to-nearest-even is exercised;
  act     oscale = 2^-e, e per (n, o) from {e0 - 1 .. e0 + 2}, e0 = round(log2(std(acc) / 4)); the same bias; lrelu slope
          0.25, gain 2, clamp 16, out_mul 0.5.  The pre-activation has a standard deviation of 1 .. 8 depending on e, so a
          few percent clamp, about half are negative.
The exponents differ between samples on purpose: an epilogue that applies the oscale row of another sample fails.

Reference: F.conv2d in fp64 on the lattice, once per row (cached on disk when a cache directory is given, so the
children of the GPU test share it), then the epilogue in fp64.  Expected stored values: the reference itself for f32,
ref.to(bfloat16) / ref.to(float16) (round to nearest even) for the 16-bit types.  Padded output channels hold
epilogue(bias[o]) because their weight rows are zero.

Case table: ROWS (geometry per row id) and PLAN (knob environment -> row id -> the plan-name stem the row is there
for).  The host test asks the library's planner, in one child process per environment, that every row still runs the
instance it declares and that the table reaches every name in ALL_DIRECT_NAMES (58) and Winograd tiles of both kinds.
Together the rows cover: each 4-stage tile unsplit (K < 512) and split-K; K / 32 = 1, 2, 3, 5 on those tiles and
K / 64 = 1, 2, 3 on both 8-phase tiles; h != w; ho * wo no multiple of 16 at n >= 2; 2 x 2 and 1-row images; pads 0, 1,
2; cout_valid < cout_p; a partial last o-tile.
"""
import collections
import os
import zlib

import torch
import torch.nn.functional as F

Row = collections.namedtuple("Row", "n h w cin_p cout_p cout_valid k pad cin")


def _r(n, h, w, cin_p, cout_p, cout_valid, k, pad, cin=None):
    return Row(n, h, w, cin_p, cout_p, cout_valid, k, pad, cin or cin_p)


def _pad32(c):
    return (c + 31) // 32 * 32


ROWS = {
    # small 3x3: h != w, ho * wo = 143 (no multiple of 16) at n = 3, cout_valid < cout_p, K = 288 (unsplit)
    "s3a": _r(3, 13, 11, 32, 64, 40, 3, 1),
    "s3b": _r(2, 7, 9, 64, 96, 96, 3, 2),          # pad 2, K = 576 (split-K), 96 = a partial 64- / 128- / 256-wide o-tile
    "s3c": _r(2, 9, 9, 1024, 256, 256, 3, 1),      # the deepest K: 9216
    "s3d": _r(3, 12, 12, 512, 512, 512, 3, 1),
    "s3e": _r(2, 10, 10, 256, 384, 362, 3, 2),     # 362 of 384 channels, pad 2
    "s3f": _r(8, 2, 2, 512, 512, 512, 3, 1),       # 2 x 2 images: every 16-pixel MFMA column spans four samples
    "s3g": _r(1, 1, 40, 64, 64, 64, 3, 1),         # a 1-row image
    # 1x1, pad 0, 63 pixels per sample: K / 32 = 1, 2, 3, 5 against the 4-deep ring (the 2-deep one of the f32 tile)
    "p32": _r(2, 9, 7, 32, 64, 64, 1, 0),
    "p64": _r(2, 9, 7, 64, 64, 40, 1, 0),
    "p96": _r(2, 9, 7, 96, 32, 32, 1, 0),
    "p160": _r(2, 9, 7, 160, 320, 300, 1, 0),      # several o-tiles, the last one partial
    # 1x1: K / 64 = 1, 2, 3 on the 8-phase tiles, whose prologue stages two K-tiles
    "q64": _r(2, 9, 7, 64, 256, 256, 1, 0),
    "q128": _r(2, 9, 7, 128, 256, 200, 1, 0),
    "q192": _r(2, 9, 7, 192, 384, 362, 1, 0),
    "p1k": _r(2, 11, 5, 1024, 1024, 1024, 1, 0),   # a 1x1 that splits K
    # the large rows (NHWC output only): tail split, 256 + 128 two-launch form, one 64-deep K-tile through the 8 phases
    "tail": _r(12, 62, 62, 128, 512, 512, 3, 1),
    "two": _r(8, 88, 88, 128, 384, 362, 3, 2),
    "k1": _r(2, 182, 181, 64, 256, 256, 1, 0),
    # halo direct conv: needs n ho wo >= 65 536
    "hc32_32": _r(2, 182, 181, 32, 32, 20, 3, 1),
    "hc32_64": _r(2, 182, 181, 32, 64, 64, 3, 2),
    "hc64_32": _r(2, 182, 181, 64, 32, 32, 3, 1),
    "hc64_64": _r(2, 182, 181, 64, 64, 51, 3, 1),
    "hc96_32": _r(2, 182, 181, 96, 32, 32, 3, 2),
    "hc96_64": _r(2, 182, 181, 96, 64, 64, 3, 1),
    # ToRGB: NCHW f32 output only
    "rgb32": _r(2, 9, 9, 32, 32, 3, 1, 0),
    "rgb64": _r(2, 9, 9, 64, 32, 4, 1, 0),
    "rgb128": _r(2, 9, 9, 128, 32, 3, 1, 0),
}
# hg4: the geometries of test_gpu_kernels.py::HG4_CASES (cin, cout, size, pad) at n = 2
HG4_CASES = [(64, 128, 45, 2), (96, 128, 40, 1), (128, 181, 40, 2), (192, 192, 33, 1), (256, 256, 30, 2),
             (32, 256, 29, 1), (128, 384, 20, 1), (64, 320, 21, 1), (181, 128, 37, 2), (81, 51, 37, 2), (64, 64, 33, 1),
             (384, 128, 24, 1), (512, 192, 21, 1)]
for _ci, _co, _s, _p in HG4_CASES:
    ROWS["h%d_%d" % (_ci, _co)] = _r(2, _s, _s, _pad32(_ci), _pad32(_co), _co, 3, _p, cin=_ci)
# the 250-wide hg4 row of test_gpu_act_blocked.py (a large row): seven whole 32-pixel x-tiles and a partial one, three
# K blocks, 90 of 96 input and 100 of 128 output channels
ROWS["h250"] = _r(2, 250, 250, 96, 128, 100, 3, 1, cin=90)
# Winograd: test_gpu_wino.py::CASES (n, cin, cout, size, pad) and one odd-width row per IC2_WINO_FLAT mode
WINO_CASES = [(2, 32, 32, 9, 2), (2, 64, 96, 13, 1), (3, 128, 160, 20, 2), (1, 512, 512, 36, 2), (2, 96, 64, 33, 0),
              (2, 256, 384, 52, 2)]
for _n, _ci, _co, _s, _p in WINO_CASES:
    ROWS["w%d_%d" % (_ci, _co)] = _r(_n, _s, _s, _pad32(_ci), _pad32(_co), _co, 3, _p, cin=_ci)
ROWS["wodd0"] = _r(2, 11, 13, 64, 64, 40, 3, 2)       # 15 x 13 outputs
ROWS["wodd1"] = _r(2, 9, 21, 96, 160, 130, 3, 1, cin=90)   # 21 x 9 outputs, two o-tiles, the second partial
ROWS["wodd2"] = _r(2, 13, 13, 64, 160, 130, 3, 2, cin=60)  # 15 x 15 outputs on a flat (wrapping) tile
# the deepest Winograd K (3 * 1024 products per accumulator); its sums are the largest of the table, so most of the
# `linear` values that f16 cannot hold come from here (test_conv_lattice_host.py, 16-bit rounding shares)
ROWS["wdeep"] = _r(2, 46, 46, 1024, 384, 384, 3, 2)

LARGE = ("tail", "two", "k1", "h250")     # one launch per dtype: act, NHWC (h250: and its blocked-input run)
HCONV = tuple(r for r in ROWS if r.startswith("hc"))   # 66 000 pixels each: five launches per dtype
TORGB = ("rgb32", "rgb64", "rgb128")
WINO = tuple(r for r in ROWS if r.startswith("w"))

# knob environments (all under IC2_DEV=1; read once per process, so one child process each)
ENVS = {"default": {}, "hg4": {"IC2_HG4": "2"}, "f32": {}, "wino": {}, "wino_flat0": {"IC2_WINO_FLAT": "0"},
        "wino_flat2": {"IC2_WINO_FLAT": "2"}}
for _t in range(1, 8):
    ENVS["tile%d" % _t] = {"IC2_IGEMM_TILE": str(_t)}


def dtypes_of(env):
    return ("f32",) if env == "f32" else ("f16",) if env.startswith("wino") else ("bf16", "f16")


JOBS = [(e, d) for e in ENVS for d in dtypes_of(e)]

TILE_STEMS = {0: "igemm_f32_128x128", 1: "igemm_256x256", 2: "igemm_32x256", 3: "igemm_128x256", 4: "igemm_128x128",
              5: "igemm_64x256", 6: "igemm8_og2", 7: "igemm8_og1"}
_SMALL = ("s3a", "s3b", "s3c", "s3d", "s3e", "s3f", "s3g", "p32", "p64", "p96", "p160", "p1k")


def _k(rid):
    r = ROWS[rid]
    return r.k * r.k * r.cin_p


# PLAN[env][row id] = the plan-name stem the row is there for (bf16 name; f16 operands append "_f16")
PLAN = {
    "default": {
        "s3a": "igemm_128x128", "s3b": "igemm_128x128_splitk", "s3c": "igemm8_og2_splitk", "s3d": "igemm8_og2_splitk",
        "s3e": "igemm_128x128_splitk", "s3f": "igemm8_og2_splitk", "s3g": "igemm_128x128_splitk",
        "p32": "igemm_128x128", "p64": "igemm_128x128", "p96": "igemm_32x256", "p160": "igemm_128x128",
        "p1k": "igemm_128x128_splitk", "tail": "igemm8_og2_tail", "two": "igemm8_og2+og1", "k1": "igemm8_og2",
        "hc32_32": "hconv_32_32", "hc32_64": "hconv_32_64", "hc64_32": "hconv_64_32", "hc64_64": "hconv_64_64",
        "hc96_32": "hconv_96_32", "hc96_64": "hconv_96_64", "rgb32": "torgb", "rgb64": "torgb", "rgb128": "torgb"},
    "hg4": {
        "h64_128": "hg4_o128_w16_s4", "h96_128": "hg4_o128_w16_s4", "h128_181": "hg4_o192_w16_s4",
        "h192_192": "hg4_o192_w16_s4", "h256_256": "hg4_o128_w32_p2", "h32_256": "hg4_o128_w32_p2",
        "h128_384": "hg4_o96_w32_p2", "h64_320": "hg4_o64_w32_p3", "h181_128": "hg4_o128_w16_s4",
        "h81_51": "hg4_o64_w16_s4", "h64_64": "hg4_o64_w16_s4", "h384_128": "hg4_o128_w32_p2",
        "h512_192": "hg4_o96_w32_p2", "h250": "hg4_o128_w32_p2",
        # 2 x 2 and 1-row images and the 143-pixel samples on the halo GEMM too
        "s3a": "hg4_o64_w16_s4", "s3f": "hg4_o128_w32_p2", "s3g": "hg4_o64_w32_p3"},
    # the exact-f32 tile (f32 operands): unsplit below K = 512, split-K from there
    "f32": {rid: "igemm_f32_128x128" + ("_splitk" if _k(rid) >= 512 else "")
            for rid in ("s3a", "s3b", "s3d", "s3e", "s3f", "s3g", "p32", "p64", "p96", "p160", "p1k")},
}
# a forced 4-stage tile: every small row; ig_plan splits K once K >= 512 (these grids are far below 320 workgroups)
for _t in range(1, 6):
    PLAN["tile%d" % _t] = {rid: TILE_STEMS[_t] + ("_splitk" if _k(rid) >= 512 else "") for rid in _SMALL}
# a forced 8-phase tile runs unsplit; it needs cin_p % 64 == 0 (other rows fall to the 256 x 256 4-stage tile)
for _t in (6, 7):
    PLAN["tile%d" % _t] = {rid: TILE_STEMS[_t] for rid in ("s3b", "s3c", "s3d", "s3e", "s3f", "s3g", "p64", "q64",
                                                            "q128", "q192", "p1k")}
# Winograd rows: PLAN names the tile, "wino_fx_o128_p<pairs>x<rows>[w]" (w: a flat tile)
PLAN["wino"] = {"w32_32": "wino_fx_o128_p16x6", "w64_96": "wino_fx_o128_p16x7", "w128_160": "wino_fx_o128_p16x8",
                "w512_512": "wino_fx_o128_p16x8", "w96_64": "wino_fx_o128_p16x8", "w256_384": "wino_fx_o128_p16x8",
                "wodd1": "wino_fx_o128_p16x5", "wdeep": "wino_fx_o128_p16x8"}
PLAN["wino_flat0"] = {"wodd0": "wino_fx_o128_p16x7", "w32_32": "wino_fx_o128_p16x6", "w512_512": "wino_fx_o128_p16x8"}
PLAN["wino_flat2"] = {"wodd2": "wino_fx_o128_p8x15w", "w32_32": "wino_fx_o128_p8x11w", "w64_96": "wino_fx_o128_p8x13w",
                      "w128_160": "wino_fx_o128_p11x11w", "w512_512": "wino_fx_o128_p20x6w"}

# every name ic2_conv_plan can return for bf16, f16 and f32 operands
_STEMS16 = ([TILE_STEMS[t] for t in range(1, 8)] + [TILE_STEMS[t] + "_splitk" for t in range(1, 6)] +
            ["igemm8_og2_splitk", "igemm8_og2_tail", "igemm8_og2+og1", "torgb"] +
            ["hg4_o64_w32_p3", "hg4_o64_w16_s4", "hg4_o96_w32_p2", "hg4_o128_w32_p2", "hg4_o128_w16_s4",
             "hg4_o192_w16_s4"] + ["hconv_%d_%d" % (i, o) for i in (32, 64, 96) for o in (32, 64)])
ALL_DIRECT_NAMES = sorted(["igemm_f32_128x128", "igemm_f32_128x128_splitk"] + _STEMS16 + [s + "_f16" for s in _STEMS16])

# ------------------------------------------------------------------ codes (ic2ops.h; no import of the package here)
F32, BF16, F16, F16_IEEE = 0, 1, 2, 5
NHWC, NCHW, NHWC16 = 0, 1, 2
DTYPE_CODE = {"f32": F32, "bf16": BF16, "f16": F16}
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
OUT_TORCH = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16, F16_IEEE: torch.float16}
EPILOGUES = {"none": dict(act=0, slope=0.0, gain=1.0, clamp=-1.0, out_mul=1.0),
             "linear": dict(act=0, slope=0.0, gain=1.0, clamp=-1.0, out_mul=1.0),
             "act": dict(act=1, slope=0.25, gain=2.0, clamp=16.0, out_mul=0.5)}


def plan_name(env, rid, dtype):
    """The full plan name row `rid` declares under `env` for operand dtype `dtype` ("bf16" / "f16" / "f32")."""
    stem = PLAN[env][rid]
    return stem + "_f16" if dtype == "f16" else stem


def plan_query(rid, dtype):
    """(dtype, out_dtype, out_layout, n, h, w, cin_p, cout_p, cout_valid, kh, kw, pad): ic2_conv_plan's arguments."""
    r = ROWS[rid]
    odt, lay = (F32, NCHW) if rid in TORGB else (DTYPE_CODE[dtype], NHWC)
    return (DTYPE_CODE[dtype], odt, lay, r.n, r.h, r.w, r.cin_p, r.cout_p, r.cout_valid, r.k, r.k, r.pad)


def variants(rid, dtype):
    """The (epilogue, out dtype code, out layout) combinations row `rid` runs for operand dtype `dtype`, each one that
    conv_check_call accepts (NCHW is f32 only).  First `act` with NHWC output in the operand dtype.  The three LARGE rows
    stop there.  Every other row then runs the other two epilogues, the other output types and the other layouts, so
    every instance sees each of them: six more launches, or four for the 66 000-pixel HCONV rows.  Those store `linear`
    as bf16 only: with K <= 864 their sums stay below 256 * 2^e, f16 holds every such m / 8 and would round nothing
    (hconv.hip stores through ig_store4v, conv_common.h, the helper whose f16 conversion the deep rows of the other
    families pin).  ToRGB is the NCHW f32 kernel: its three epilogues."""
    if rid in TORGB:
        return [("act", F32, NCHW), ("none", F32, NCHW), ("linear", F32, NCHW)]
    base = [("act", DTYPE_CODE[dtype], NHWC)]
    if rid in LARGE:
        return base
    if rid in HCONV:   # every epilogue, layout and output type once; `linear` is stored as bf16, not as f16
        return base + [("none", F16_IEEE, NHWC16), ("linear", F32, NCHW), ("none", BF16 if dtype != "bf16" else F16, NHWC),
                       ("linear", BF16, NHWC)]
    return base + [("none", F32, NHWC), ("linear", BF16, NHWC16), ("linear", F16, NHWC), ("none", F16_IEEE, NHWC16),
                   ("linear", F32, NCHW), ("act", BF16 if dtype != "bf16" else F16, NHWC16)]


def _gen(rid, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(rid.encode()) + salt)


def operands(rid):
    """(x [n][h][w][cin_p], w [cout_p][k][k][cin_p]) as float32 tensors holding the lattice integers."""
    r = ROWS[rid]
    g = _gen(rid)
    x = torch.randint(-4, 5, (r.n, r.h, r.w, r.cin_p), generator=g).float()
    w = torch.randint(-2, 3, (r.cout_p, r.k, r.k, r.cin_p), generator=g).float()
    if rid in WINO:
        w = w * 2
    x[..., r.cin:] = 0
    w[..., r.cin:] = 0
    w[r.cout_valid:] = 0
    return x, w


def wino_weight_oihw(w, r):
    """The Winograd pack's input: the valid part of the packed lattice weight as [cout][cin][3][3] f32."""
    return w[:r.cout_valid, :, :, :r.cin].permute(0, 3, 1, 2).contiguous()


CACHE_MIN_ELEMENTS = 1 << 21   # smaller accumulators recompute in milliseconds and are not written to the cache


def conv_acc(rid, cache_dir=None):
    """The fp64 convolution of the row's lattice, NHWC [n][ho][wo][cout_p], computed once per row.  With `cache_dir` the
    accumulators of the rows of at least CACHE_MIN_ELEMENTS outputs (the large, hconv and deep Winograd rows: 17 - 200
    MB each, about 0.9 GB together) are kept there for the other child processes."""
    r = ROWS[rid]
    numel = r.n * (r.h + 2 * r.pad - r.k + 1) * (r.w + 2 * r.pad - r.k + 1) * r.cout_p
    path = os.path.join(cache_dir, rid + ".acc.pt") if cache_dir and numel >= CACHE_MIN_ELEMENTS else None
    if path and os.path.exists(path):
        return torch.load(path)
    x, w = operands(rid)
    acc = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), padding=r.pad)
    acc = acc.permute(0, 2, 3, 1).contiguous()
    if path:
        torch.save(acc, path + ".tmp%d" % os.getpid())
        os.replace(path + ".tmp%d" % os.getpid(), path)
    return acc


def epilogue_params(rid, epi, acc):
    """(oscale [n][cout_p] f32 or None, bias [cout_p] f32 or None) of epilogue `epi` (module docstring)."""
    if epi == "none":
        return None, None
    r = ROWS[rid]
    g = _gen(rid, 1 if epi == "linear" else 2)
    e = torch.randint(0, 4, (r.n, r.cout_p), generator=g)
    bias = torch.randint(-16, 17, (r.cout_p,), generator=g).float() / 8
    if epi == "act":
        std = acc[..., :r.cout_valid].std().item()
        e = e - 1 + int(round(torch.log2(torch.tensor(std / 4)).item()))
    return torch.pow(2.0, -e.double()).float(), bias


def apply_epilogue(acc, epi, oscale, bias):
    """ic2ops.h's epilogue in fp64 on the NHWC accumulator."""
    p = EPILOGUES[epi]
    v = acc
    if oscale is not None:
        v = v * oscale.double()[:, None, None, :] + bias.double()[None, None, None, :]
    if p["act"]:
        v = (torch.where(v < 0, v * p["slope"], v) * p["gain"]).clamp(-p["clamp"], p["clamp"])
    return v * p["out_mul"]


def to_layout(v, layout, cout_valid):
    """NHWC [n][ho][wo][cout_p] -> the stored layout."""
    n, ho, wo, cp = v.shape
    if layout == NCHW:
        return v[..., :cout_valid].permute(0, 3, 1, 2).contiguous()
    if layout == NHWC16:
        return v.reshape(n, ho, wo, cp // 16, 16).permute(0, 3, 1, 2, 4).contiguous()
    return v


def from_layout(y, layout):
    """The stored layout -> NHWC (NCHW: its cout_valid channels)."""
    if layout == NCHW:
        return y.permute(0, 2, 3, 1)
    if layout == NHWC16:
        n, cb, ho, wo, _ = y.shape
        return y.permute(0, 2, 3, 1, 4).reshape(n, ho, wo, cb * 16)
    return y


def expected(ref, out_code, layout, cout_valid):
    """The stored tensor: `ref` (fp64, exactly representable in f32) rounded to nearest even into the output type."""
    v = ref.float()
    if out_code == F16:  # activations saturate at the f16 range (the lattice never reaches it)
        v = v.clamp(-65504.0, 65504.0)
    return to_layout(v.to(OUT_TORCH[out_code]), layout, cout_valid)


def first_difference(got, exp, layout):
    """"" when the tensors are equal, else the count of differing elements and the first (n, y, x, o) with both values."""
    if torch.equal(got, exp):
        return ""
    g, e = from_layout(got, layout).float(), from_layout(exp, layout).float()
    bad = (g != e) | (g.isnan() != e.isnan())
    idx = bad.nonzero()[0].tolist()
    return "%d of %d elements differ, first at (n, y, x, o) = %s: got %r, expected %r" % (
        int(bad.sum()), bad.numel(), tuple(idx), g[tuple(idx)].item(), e[tuple(idx)].item())


# ------------------------------------------------------------------ rounding tier (Gaussian operands)
# family -> (env, row id, operand dtype): one small row per kernel family (hconv has no small geometry)
ROUNDING = {"igemm": ("default", "s3a", "bf16"), "igemm_splitk": ("default", "s3b", "f16"),
            "igemm8": ("tile6", "s3b", "bf16"), "hg4": ("hg4", "h81_51", "f16"), "hconv": ("default", "hc32_32", "bf16"),
            "f32": ("f32", "s3a", "f32"), "wino": ("wino", "w64_96", "f16")}
EPS = {"wino": 2.0 ** -11}   # U and V are rounded to f16; every other family: exact products, f32 sums
EPS_OUT = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}
G_MAT = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
BT_MAT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
AT_MAT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def gaussian_case(rid, dtype):
    """Gaussian operands rounded to the storage type, a Gaussian `linear` epilogue, the fp64 reference and the magnitude
    bound B = |oscale| conv(|x|, |w|) + |bias| (Winograd: propagated through |B^T|, |G|, |A^T|), all NHWC."""
    r = ROWS[rid]
    g = _gen(rid, 3)
    td = TORCH_DTYPE[dtype]
    x = torch.randn(r.n, r.h, r.w, r.cin_p, generator=g)
    w = torch.randn(r.cout_p, r.k, r.k, r.cin_p, generator=g) / (r.k * r.k * r.cin) ** 0.5
    x[..., r.cin:] = 0
    w[..., r.cin:] = 0
    w[r.cout_valid:] = 0
    if rid not in WINO:   # (the Winograd pack takes the f32 weight and rounds U itself)
        w = w.to(td).float()
    x = x.to(td).float()
    oscale = (torch.randn(r.n, r.cout_p, generator=g).abs() + 0.5) * torch.where(
        torch.rand(r.n, r.cout_p, generator=g) < 0.5, -1.0, 1.0)
    bias = torch.randn(r.cout_p, generator=g)
    xd, wd = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    acc = F.conv2d(xd, wd, padding=r.pad).permute(0, 2, 3, 1)
    ref = acc * oscale.double()[:, None, None, :] + bias.double()
    if rid in WINO:
        ho, wo = acc.shape[1:3]
        u_abs = torch.einsum("uk,ocyk->ocyu", G_MAT.abs(), wd.abs())                  # |G| |w| per (o, c, ky, nu)
        xp = F.pad(xd.abs(), (r.pad, r.pad + 2, r.pad, r.pad))                        # room for the last pair
        m = []
        for nu in range(4):
            kern = u_abs[..., nu, None] * BT_MAT[nu].abs()                             # [o][c][3][4]
            m.append(F.conv2d(xp, kern, stride=(1, 2)))
        m = torch.stack(m, -1)                                                        # [n][o][ho][pairs][4]
        yb = torch.einsum("ju,nohpu->nohpj", AT_MAT.abs(), m).reshape(m.shape[0], m.shape[1], m.shape[2], -1)
        cabs = yb[..., :ho, :wo].permute(0, 2, 3, 1)
    else:
        cabs = F.conv2d(xd.abs(), wd.abs(), padding=r.pad).permute(0, 2, 3, 1)
    bound = cabs * oscale.double().abs()[:, None, None, :] + bias.double().abs()
    return dict(x=x, w=w, oscale=oscale, bias=bias, ref=ref.contiguous(), B=bound.contiguous())
