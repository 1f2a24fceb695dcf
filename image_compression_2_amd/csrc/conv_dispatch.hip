// The conv dispatcher: no device code.  conv_choice computes one ConvPlan (conv_plan.h) per call -- kernel family, tile
// instance, split forms, workspace bytes -- and the launch (ic2_conv_igemm_ws), the plan-name query (ic2_conv_plan), the
// workspace query (ic2_conv_igemm_ws_bytes), the layout query (ic2_conv_accepts_nhwc16) and the fused conv + GroupNorm
// path (conv_gn_*) all read that plan, so what is tested and timed is what runs.  Nothing re-derives a decision after
// it; the one downgrade is ic2_conv_igemm_ws dropping a split form when the caller's workspace is missing or short.
// The kernels and their launchers: igemm.hip, igemm8.hip, hg4.hip, hconv.hip (and wino.hip behind its own entry point).
#include "conv_plan.h"

#include <cstdlib>

namespace ic2 {

// hg4 instance: o-tile 96 when cout_p % 192 == 0 (two 96-wide o-tiles on 8 x 32-pixel tiles: a weight slab feeds 256
// pixels instead of the 192-wide tile's 128, so 2.1 instead of 3.4 LDS-DMA pieces per 24 MFMAs; SG3-T-256 L11
// 2.27 -> 2.15 ms, profiles/r4x_hg4_o96.txt), 128 when cout_p % 128 == 0, else 64.  Pixel tile 32 or 16 wide,
// whichever pads the output less (a 96-wide o-tile whose output pads less on 16-wide tiles runs as the 192-wide
// 16-wide-tile instance).
static H4Plan h4_plan(int n, int ho, int wo, int cout_p) {
  H4Plan p;
  p.bo = cout_p % 192 == 0 ? 96 : cout_p % 128 == 0 ? 128 : 64;
  const int th32 = 8, th16 = p.bo != 96 ? 16 : 8;  // 256-pixel tiles; 128 pixels under the 192-wide o-tile
  const int64_t a32 = ceil_div(ho, th32) * th32 * ceil_div(wo, 32) * 32;
  const int64_t a16 = ceil_div(ho, th16) * th16 * ceil_div(wo, 16) * 16;
  p.tw32 = a32 <= a16;
  if (p.bo == 96 && !p.tw32) p.bo = 192;
  p.th = p.tw32 ? th32 : th16;
  p.tw = p.tw32 ? 32 : 16;
  p.area = p.tw32 ? a32 : a16;
  p.blocks = n * (p.area / (p.th * p.tw)) * ceil_div(cout_p, p.bo);
  return p;
}

// bf16 3x3 with 32-deep channel blocks.  Default: on a grid of >= 2 workgroups per CU, <= 512 channels in, <= 192
// out, >= 93 % pixel-tile utilisation (tools/sweep_igemm.py, profiles/r2e_hg4_sweep.txt).  Knob IC2_HG4 (IC2_DEV=1):
// 0 disables it, 2 forces it wherever legal (the tests' forced-instance runs).
static bool hg4_legal(int dtype, int cin_p, int cout_p, int kh, int kw, int64_t x_elems) {
  return is16(dtype) && kh == 3 && kw == 3 && cin_p % 32 == 0 && cout_p % 64 == 0 &&
         x_elems * 2 < (int64_t)kOob && (int64_t)cout_p * 9 * cin_p * 2 < (int64_t)kOob;
}
static bool hg4_by_default(const H4Plan& p, int cin_p, int cout_p, int ho, int wo) {
  if (p.blocks < 512) return false;
  const double util = (double)ho * wo / (double)p.area;
  // inputs up to 512 channels (the split encoder's 384-wide block-1 conv2: og1 -> hg4 + fused statistics, C4
  // +1.1 %, profiles/r3_hg4_maxc_ab.txt)
  return cin_p <= 512 && cout_p <= 192 && util >= 0.93;
}

// ------------------------------------------------------------------------------------------------
// implicit-GEMM tile instance (kIgTiles, conv_plan.h) and K split.
// Knob (IC2_DEV=1 only): IC2_IGEMM_TILE=1..7 forces a bf16 tile (the tests exercise every instance on small
// problems).
static void ig_plan(ConvPlan& c, int dtype, int64_t M, int cout_p, int cin_p, int kh, int kw, int64_t x_elems, bool x8) {
  static const int forced = knob("IC2_IGEMM_TILE", 0);
  const int64_t K = (int64_t)kh * kw * cin_p;
  int tile = IG_F32_128x128;
  c.splits = 1;
  c.tail = false;
  if (is16(dtype)) {
    // o-tile: the widest of {256, 128, 64, 32} that divides cout_p (no padded MFMA rows), 256-pixel
    // tiles while the grid keeps >= 2 workgroups per CU, else the 128 x 128 tile
    const bool big_m = ceil_div(M, 256) * ((cout_p + 255) / 256) >= 512;
    if (!big_m) tile = cout_p <= 32 ? IG_32x256 : IG_128x128;
    else if (cout_p % 256 == 0) tile = IG_256x256;
    else if (cout_p % 128 == 0) tile = IG_128x256;
    else if (cout_p % 64 == 0) tile = IG_64x256;
    else tile = IG_32x256;
    // the 8-phase kernels wherever K-tiles are 64 deep (their buffer descriptors address < 2 GiB per
    // operand and their tap masks hold <= 32 taps) and the grid keeps ~1 workgroup per CU (measured on the
    // bench shapes, tools/sweep_igemm.py): 256 x 256 for cout_p > 128 (padded 64-row quadrants skip their
    // MFMAs) unless cout_p is an odd multiple of 128 (384: the 128 x 512 tile pads nothing), 128 x 512 for
    // 64 < cout_p <= 128; cout_p = 64 keeps the 64 x 256 tile
    const bool fits8 = x8 && cin_p % 64 == 0 && kh * kw <= 32 && x_elems * 2 < (int64_t)kOob &&
                       (int64_t)cout_p * K * 2 < (int64_t)kOob;
    const bool odd128 = cout_p % 256 == 128 && cout_p > 128;
    // small grids (the encoder's 512-wide blocks at <= 32^2): the same 8-phase tiles with K split over
    // gridDim.y so the launch reaches ~1 workgroup per CU, instead of the 4-stage 128 x 128 split-K tile
    const int64_t g6 = ceil_div(M, 256) * ((cout_p + 255) / 256), g7 = ceil_div(M, 512) * ((cout_p + 127) / 128);
    const bool k_deep = K / 64 >= 32;
    int g8_split = 1;
    // (a full-K grid of 1-2 rounds is not split for wave balance: SG3-T-256 L0-L3's 362 workgroups as 724 half-K ones
    // measured 10 % slower, the f32 partials and the combine costing more than the idle tail, r6_schedule_ab.txt)
    if (fits8 && cout_p > 128 && !odd128 && g6 >= 240) tile = IG_G8_OG2;
    else if (fits8 && (odd128 || (cout_p > 64 && cout_p <= 128)) && g7 >= 240) tile = IG_G8_OG1;
    else if (fits8 && k_deep && cout_p > 128 && !odd128)
      tile = IG_G8_OG2, g8_split = (int)ceil_div(240, g6);  // aims at ~1 workgroup per CU
    if (g8_split > 1) {
      int64_t sp = g8_split;
      if (sp > K / 64 / 8) sp = K / 64 / 8;  // >= 8 K-tiles of 64 per slice
      if (sp > 32) sp = 32;
      g8_split = M * cout_p < (1LL << 31) ? (int)sp : 1;
    }
    if (forced >= 1 && forced <= 7) tile = forced, g8_split = 1;
    if ((tile == IG_G8_OG2 || tile == IG_G8_OG1) && !fits8) tile = IG_256x256, g8_split = 1;
    c.splits = g8_split;
  }
  c.tile = tile;
  if (c.splits > 1) return;
  // Wave balance of a full-K 256 x 256 grid (one workgroup per CU on 256 CUs): a last round of r <= 128 tiles runs as
  // 2r half-K workgroups -- one round of half the time -- behind a launch of the whole rounds; the tail's f32 partials
  // are combined over its pixels only (SG3-T-256 L0-L2 at batch 32: 362 tiles = 256 + 106, 2 rounds -> 1.5).  Round 6
  // split every tile of such a grid instead (724 half-K workgroups: 10 % slower, every tile paying the partials).
  // The tail's pixels are those of its p-tiles in the p-tile-major tile order (tile_coords, group 1).
  if (tile == IG_G8_OG2 && K / 64 >= 16 && M * cout_p < (1LL << 31)) {
    const int64_t tiles_o = (cout_p + 255) / 256, tiles = ceil_div(M, 256) * tiles_o, rem = tiles % 256;
    if (tiles > 256 && rem > 0 && rem <= 128 && (tiles - rem) % tiles_o == 0) c.tail = true;
  }
  if (tile < IG_G8_OG2) {
    // fewer workgroups than ~1.25 per CU: split K so the launch reaches ~512 workgroups, each slice
    // keeping >= 8 chunks of 32
    const int64_t blocks = ceil_div(M, kIgTiles[tile].bp) * ceil_div(cout_p, kIgTiles[tile].bo);
    const int64_t nq32 = K / 32;
    if (blocks < 320 && M * cout_p < (1LL << 31)) {
      int64_t sp = ceil_div(512, blocks);
      if (sp > nq32 / 8) sp = nq32 / 8;
      if (sp > 32) sp = 32;
      c.splits = sp < 1 ? 1 : (int)sp;
    }
  }
}

// the halo kernel for bf16 3x3 convs with cin_p in {32, 64, 96}, cout_p in {32, 64} and >= 64K output pixels
static bool hconv_eligible(int dtype, int64_t M, int cin_p, int cout_p, int kh, int kw) {
  return is16(dtype) && kh == 3 && kw == 3 && (cin_p == 32 || cin_p == 64 || cin_p == 96) &&
         (cout_p == 32 || cout_p == 64) && M >= 65536;
}

// (the ToRGB kernel maps output pixel p to input pixel p: 1x1, no padding)
static bool torgb_eligible(int dtype, int cin_p, int cout_valid, int kh, int kw, int pad, int out_layout,
                           int out_dtype) {
  return is16(dtype) && kh == 1 && kw == 1 && pad == 0 && cout_valid <= 4 && out_layout == IC2_LAYOUT_NCHW &&
         out_dtype == IC2_F32 && (cin_p == 32 || cin_p == 64 || cin_p == 128);
}

// stored elements per input pixel: the split-bf16 input (IC2_BF16X3, cin_p = the GEMM's tripled K channels) is
// stored [hi | lo], 2/3 of them; the f16 input of the split-weight mode (IC2_F16X2, cin_p = the doubled K) half
static int x_pix_of(int dtype, int cin_p) {
  return dtype == IC2_BF16X3 ? cin_p / 3 * 2 : dtype == IC2_F16X2 ? cin_p / 2 : cin_p;
}
// 32-channel blocks of the stored input the split K runs over twice (hi, hi) / once more (x, x) (0: plain input)
static int x_hb32_of(int dtype, int cin_p) { return dtype == IC2_BF16X3 ? cin_p / 96 : dtype == IC2_F16X2 ? cin_p / 64 : 0; }

// The launch plan of one launch (n = the images of the launch, see conv_chunk_n).
static ConvPlan conv_choice(int dtype, int out_layout, int out_dtype, int n, int h, int w_, int cin_p, int cout_p,
                            int cout_valid, int kh, int kw, int pad) {
  const int ho = h + 2 * pad - kh + 1, wo = w_ + 2 * pad - kw + 1;
  const int64_t M = (int64_t)n * ho * wo;
  const int64_t x_elems = (int64_t)n * h * w_ * x_pix_of(dtype, cin_p);  // stored elements (buffer-offset limits)
  ConvPlan c{};
  // the split inputs (IC2_BF16X3 [hi | lo] storage, IC2_F16X2 plain f16) run on the kernels whose input addressing
  // maps the tripled / doubled K onto them (implicit GEMM, 8-phase, hg4), planned as the 16-bit GEMM over that K.
  // The 8-phase kernels address 64-channel K blocks: the doubled K needs an even number of stored 32-channel blocks
  const bool x3 = dtype == IC2_BF16X3 || dtype == IC2_F16X2;
  const bool x8 = dtype != IC2_F16X2 || (cin_p / 2) % 64 == 0;
  if (x3) dtype = dtype == IC2_F16X2 ? IC2_F16 : IC2_BF16;
  // hg4 ahead of the halo direct conv for >= 96 input channels (SG3-T-1024 L11: 1532 -> 1363 us at batch 8); the
  // 32 / 64-channel encoder layers stay on hconv (faster there)
  static const int hg4_mode = knob("IC2_HG4", 1);
  bool hg4_ok = hg4_mode && hg4_legal(dtype, cin_p, cout_p, kh, kw, x_elems);
  if (hg4_ok) {
    c.h4 = h4_plan(n, ho, wo, cout_p);
    hg4_ok = hg4_mode == 2 || hg4_by_default(c.h4, cin_p, cout_p, ho, wo);
  }
  const bool hg4_pref = cin_p >= 96;
  if (!x3 && torgb_eligible(dtype, cin_p, cout_valid, kh, kw, pad, out_layout, out_dtype)) c.kind = CK_TORGB;
  else if (hg4_ok && hg4_pref) c.kind = CK_HG4;
  else if (!x3 && hconv_eligible(dtype, M, cin_p, cout_p, kh, kw)) c.kind = CK_HCONV;
  else if (hg4_ok) c.kind = CK_HG4;
  else c.kind = CK_IGEMM;
  c.splits = 1;
  c.hc_cin = cin_p;
  c.hc_cout = cout_p;
  if (c.kind != CK_IGEMM) return c;
  ig_plan(c, dtype, M, cout_p, cin_p, kh, kw, x_elems, x8);
  // an odd multiple of 128 above 128 (384: SG3-T-256 L9, SG3-T-1024 L7): the 256-wide tile on all but the last
  // 128 channels, the 128 x 512 tile on those (both read the same input panel)
  c.split384 = is16(dtype) && c.tile == IG_G8_OG1 && cout_p % 256 == 128 && cout_p > 128 &&
               ceil_div(M, 256) >= 240;
  if (c.tail) {  // the tail: the tiles past the whole rounds; its pixels: that tile's p-tile (p-tile-major order) on
    const int64_t tiles_o = (cout_p + 255) / 256, g6 = ceil_div(M, 256) * tiles_o;
    c.tail_tile = (int)(g6 - g6 % 256);
    c.p_lo = (int)(c.tail_tile / tiles_o * 256);
  }
  // f32 partial sums [slices][M][cout_p] of the split forms, in a caller-owned workspace
  if (c.splits > 1 || c.tail) c.ws_bytes = (int64_t)(c.tail ? 2 : c.splits) * M * cout_p * 4;
  return c;
}

// (thread_local buffer: valid until the thread's next call)
static const char* conv_choice_name(const ConvPlan& c) {
  static thread_local char buf[64];
  switch (c.kind) {
    case CK_TORGB: return "torgb";
    case CK_HCONV: snprintf(buf, sizeof(buf), "hconv_%d_%d", c.hc_cin, c.hc_cout); break;
    case CK_HG4:
      snprintf(buf, sizeof(buf), "hg4_o%d_w%s", c.h4.bo, !c.h4.tw32 ? "16_s4" : c.h4.bo == 64 ? "32_p3" : "32_p2");
      break;
    case CK_IGEMM:
      if (c.split384) return "igemm8_og2+og1";
      snprintf(buf, sizeof(buf), "%s%s", kIgTiles[c.tile].name, c.splits > 1 ? "_splitk" : c.tail ? "_tail" : "");
      break;
  }
  return buf;
}

// the kernels whose input addressing covers the channel-blocked layout (IgemmArgs::x_plane): the hg4 halo staging
// and ToRGB, on plain 2-byte operands (the split inputs have their own storage)
static bool conv_kind_reads_blocked(ConvKind kind, int dtype) {
  return (kind == CK_HG4 || kind == CK_TORGB) && (dtype == IC2_BF16 || dtype == IC2_F16);
}

// Images per launch: the buffer-descriptor kernels (8-phase, hg4) address < 2^31 bytes per operand, so a batch whose
// input exceeds that runs in chunks of whole images (each chunk with its own launch plan) instead of falling back to
// the generic tile (SG3-T-1024 / the 1024^2 encoder at batch 8: 1024^2 x 192 x 2 B = 403 MB per image).
int64_t conv_x_img_bytes(int dtype, int h, int w_, int cin_p) {
  return (int64_t)h * w_ * x_pix_of(dtype, cin_p) * (dtype == IC2_F32 ? 4 : 2);
}
int conv_chunk_n(int dtype, int n, int h, int w_, int cin_p) {
  const int64_t per_img = conv_x_img_bytes(dtype, h, w_, cin_p);
  if ((int64_t)n * per_img < (int64_t)kOob || per_img >= (int64_t)kOob) return n;
  const int64_t c = ((int64_t)kOob - 1) / per_img;
  const int64_t chunks = ceil_div(n, c);
  return (int)ceil_div(n, chunks);  // balanced chunks
}
// the plan of a call's launches: that of a chunk of *nc images
static ConvPlan conv_choice_chunked(int dtype, int out_layout, int out_dtype, int n, int h, int w_, int cin_p, int cout_p,
                                    int cout_valid, int kh, int kw, int pad, int* nc) {
  *nc = conv_chunk_n(dtype, n, h, w_, cin_p);
  return conv_choice(dtype, out_layout, out_dtype, *nc, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad);
}

// The launch arguments of a plain conv: bias only, no activation, NHWC input and output, no fused GroupNorm.  The
// callers set what differs.
IgemmArgs make_igemm_args(const void* x, const void* w, void* y, const float* bias, int dtype, int out_dtype, int n,
                          int h, int w_, int cin_p, int cout_p, int cout_valid, int kh, int kw, int pad, float out_mul) {
  IgemmArgs a{};
  a.x = x; a.w = w; a.y = y; a.bias = bias;
  a.n = n; a.h = h; a.w_ = w_; a.cin_p = cin_p; a.cout_p = cout_p; a.cout_valid = cout_valid;
  a.kh = kh; a.kw = kw; a.pad = pad; a.ho = h + 2 * pad - kh + 1; a.wo = w_ + 2 * pad - kw + 1;
  a.M = (int)((int64_t)n * a.ho * a.wo); a.K = kh * kw * cin_p; a.nq = a.K / 32;
  a.act_gain = 1.f; a.clamp = -1.f; a.out_mul = out_mul;
  a.out_layout = IC2_LAYOUT_NHWC; a.out_dtype = out_dtype;
  a.group = 1;   // p-tile-major tile order (tile_coords)
  a.korder = 1;  // channel-major K (igemm8.hip)
  a.x_pix = x_pix_of(dtype, cin_p);
  a.x_hb32 = x_hb32_of(dtype, cin_p);
  ig_set_input_layout(a, false);
  return a;
}

int conv_check_call(const char* who, ConvCall& c) {
  // the input layout rides in the bits above the activation (ic2ops.h IC2_ACT_IN_LAYOUT)
  const int in_layout = IC2_ACT_IN_LAYOUT_OF(c.act);
  c.act = IC2_ACT_OF(c.act);
  IC2_CHECK_ARG(in_layout == IC2_LAYOUT_NHWC || in_layout == IC2_LAYOUT_NHWC16, "%s: bad input layout %d", who,
                in_layout);
  c.in_blocked = in_layout == IC2_LAYOUT_NHWC16;
  IC2_CHECK_ARG(c.out_dtype == IC2_F32 || c.out_dtype == IC2_BF16 ||
                    ((c.out_dtype == IC2_F16 || c.out_dtype == IC2_F16_IEEE) && c.out_layout != IC2_LAYOUT_NCHW),
                "%s: bad out dtype %d", who, c.out_dtype);
  IC2_CHECK_ARG(c.cin_p > 0 && c.cin_p % 32 == 0 && c.cout_p > 0 && c.cout_p % 32 == 0,
                "%s: channel strides must be positive multiples of 32 (cin_p=%d cout_p=%d)", who, c.cin_p, c.cout_p);
  IC2_CHECK_ARG(c.n > 0 && c.h > 0 && c.w_ > 0 && c.kh > 0 && c.kw > 0 && c.pad >= 0, "%s: bad geometry", who);
  IC2_CHECK_ARG(c.ho == c.h + 2 * c.pad - c.kh + 1 && c.wo == c.w_ + 2 * c.pad - c.kw + 1 && c.ho > 0 && c.wo > 0,
                "%s: output size %dx%d does not match input %dx%d, k=%dx%d, pad=%d", who, c.ho, c.wo, c.h, c.w_, c.kh,
                c.kw, c.pad);
  IC2_CHECK_ARG(c.out_layout == IC2_LAYOUT_NHWC || c.out_layout == IC2_LAYOUT_NHWC16 ||
                    (c.out_layout == IC2_LAYOUT_NCHW && c.out_dtype == IC2_F32 && c.cout_valid > 0 &&
                     c.cout_valid <= c.cout_p),
                "%s: NCHW output needs f32 and 0 < cout_valid <= cout_p (layout %d)", who, c.out_layout);
  c.out_ieee = c.out_dtype == IC2_F16_IEEE;
  if (c.out_ieee) c.out_dtype = IC2_F16;
  return IC2_OK;
}

}  // namespace ic2

using namespace ic2;

extern "C" const char* ic2_conv_plan(int dtype, int out_dtype, int out_layout, int n, int h, int w_, int cin_p,
                                     int cout_p, int cout_valid, int kh, int kw, int pad) {
  const int ho = h + 2 * pad - kh + 1, wo = w_ + 2 * pad - kw + 1;
  if (n <= 0 || ho <= 0 || wo <= 0 || cin_p <= 0 || cout_p <= 0) return "invalid";
  int nc;
  const char* name = conv_choice_name(
      conv_choice_chunked(dtype, out_layout, out_dtype, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, &nc));
  if (dtype != IC2_F16 && dtype != IC2_F16X2) return name;
  static thread_local char f16_name[80];  // the f16-operand instance of the same kernel
  snprintf(f16_name, sizeof(f16_name), "%s_f16", name);
  return f16_name;
}

// The filtered lrelu -> conv hand-off stays channel-blocked where the consumer reads it that way and does not lose
// more than the filtered lrelu gains (per kernel family, profiles/r7_act_blocked_ab.txt): Winograd and hg4 do, ToRGB
// does not (+20 us against its filtered lrelu's -19 us; launching it on blocked input stays legal)
extern "C" int ic2_conv_accepts_nhwc16(int dtype, int out_dtype, int out_layout, int n, int h, int w_, int cin_p,
                                       int cout_p, int cout_valid, int kh, int kw, int pad) {
  const int ho = h + 2 * pad - kh + 1, wo = w_ + 2 * pad - kw + 1;
  if (n <= 0 || ho <= 0 || wo <= 0 || cin_p <= 0 || cin_p % 32 || cout_p <= 0 || cout_p % 32) return 0;
  if (ic2_conv_wino_preferred(dtype, n, h, w_, cin_p, cout_p, kh, kw, pad)) return 1;
  int nc;
  const ConvPlan c = conv_choice_chunked(dtype, out_layout, out_dtype, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, &nc);
  return c.kind == CK_HG4 && conv_kind_reads_blocked(c.kind, dtype);
}

extern "C" int64_t ic2_conv_igemm_ws_bytes(int dtype, int n, int h, int w_, int cin_p, int cout_p, int kh, int kw,
                                           int pad) {
  const int ho = h + 2 * pad - kh + 1, wo = w_ + 2 * pad - kw + 1;
  if (n <= 0 || h <= 0 || w_ <= 0 || ho <= 0 || wo <= 0 || cin_p <= 0 || cout_p <= 0 || kh <= 0 || kw <= 0) return 0;
  int nc;
  return conv_choice_chunked(dtype, IC2_LAYOUT_NHWC, dtype, n, h, w_, cin_p, cout_p, cout_p, kh, kw, pad, &nc).ws_bytes;
}

extern "C" int ic2_conv_igemm_ws(const void* x, const void* w, void* y, int dtype, int out_dtype, int n, int h, int w_,
                                 int cin_p, int cout_p, int cout_valid, int kh, int kw, int pad, int ho, int wo,
                                 const float* oscale, const float* bias, int act, float slope, float act_gain,
                                 float clamp, float out_mul, int out_layout, void* workspace, int64_t ws_bytes,
                                 void* stream) {
  IC2_CHECK_ARG(x && w && y, "conv_igemm: null pointer");
  IC2_CHECK_ARG(dtype == IC2_F32 || dtype == IC2_BF16 || dtype == IC2_F16 || dtype == IC2_BF16X3 || dtype == IC2_F16X2,
                "conv_igemm: bad dtype %d", dtype);
  IC2_CHECK_ARG(dtype != IC2_BF16X3 || (cin_p % 96 == 0 && out_layout == IC2_LAYOUT_NHWC),
                "conv_igemm: split-bf16 input needs cin_p = 3 x a multiple of 32 and NHWC output (cin_p=%d)", cin_p);
  IC2_CHECK_ARG(dtype != IC2_F16X2 || (cin_p % 64 == 0 && out_layout == IC2_LAYOUT_NHWC),
                "conv_igemm: split-weight f16 input needs cin_p = 2 x a multiple of 32 and NHWC output (cin_p=%d)", cin_p);
  ConvCall cc{x, w, y, oscale, bias, dtype, out_dtype, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, ho, wo,
              act, slope, act_gain, clamp, out_mul, out_layout};
  if (const int rc = conv_check_call("conv_igemm", cc)) return rc;
  IC2_CHECK_ARG(((uintptr_t)oscale | (uintptr_t)bias | (uintptr_t)workspace) % 16 == 0,
                "conv_igemm: oscale/bias/workspace must be 16-byte aligned");
  hipStream_t s = as_stream(stream);
  return conv_for_chunks(cc, [&](IgemmArgs& a) -> int {
    IC2_CHECK_ARG((int64_t)a.n * ho * wo < (1LL << 30), "conv_igemm: too many output pixels");
    a.ws = reinterpret_cast<float*>(workspace);
    ConvPlan c = conv_choice(dtype, out_layout, cc.out_dtype, a.n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad);
    IC2_CHECK_ARG(!cc.in_blocked || conv_kind_reads_blocked(c.kind, dtype),
                  "conv_igemm: channel-blocked (NHWC16) input is read by the hg4 halo kernels and ToRGB only, with "
                  "plain bf16 / f16 operands; this geometry runs as %s (ic2_conv_accepts_nhwc16 says which do)",
                  conv_choice_name(c));
    // the one downgrade of a plan: a split form without its workspace (a plan query cannot know the caller's buffer)
    if (c.ws_bytes > 0 && (workspace == nullptr || ws_bytes < c.ws_bytes)) c.splits = 1, c.tail = false, c.ws_bytes = 0;
    const bool f16 = dtype == IC2_F16 || dtype == IC2_F16X2;  // the kernels' operand type
    switch (c.kind) {
      case CK_TORGB: launch_torgb(a, f16, s); break;
      case CK_HG4: launch_hg4(a, c.h4, f16, false, s); break;
      case CK_HCONV: launch_hconv(a, f16, s); break;
      case CK_IGEMM:
        if (c.tile >= IG_G8_OG2) launch_igemm8(a, c, f16, s);
        else launch_igemm(a, c.tile, f16, c.splits, s);
        if (c.ws_bytes > 0) launch_splitk_reduce(a, c.tail ? 2 : c.splits, c.p_lo, s);
        break;
    }
    IC2_CHECK_LAUNCH("conv_igemm");
    return IC2_OK;
  });
}

extern "C" int ic2_conv_igemm(const void* x, const void* w, void* y, int dtype, int out_dtype, int n, int h, int w_,
                              int cin_p, int cout_p, int cout_valid, int kh, int kw, int pad, int ho, int wo,
                              const float* oscale, const float* bias, int act, float slope, float act_gain,
                              float clamp, float out_mul, int out_layout, void* stream) {
  return ic2_conv_igemm_ws(x, w, y, dtype, out_dtype, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, ho, wo, oscale,
                           bias, act, slope, act_gain, clamp, out_mul, out_layout, nullptr, 0, stream);
}

namespace ic2 {
// ------------------------------------------------------------------------------------------------
// conv + GroupNorm statistics (conv_plan.h): the statistics ride in the hg4 epilogue of the split modes.  The bf16 halo
// conv (hconv) had such an epilogue too; it was removed because its two extra barriers per tile of the persistent kernel
// cost what the saved read of y gained (C2 1277 -> 1256 img/s, profiles/r2b_conv_gn_ab.txt), so every other dtype runs
// the plain conv and the caller the separate statistics pass.

// rows of the statistics-epilogue kernel's pixel tile: 12 for the 64-wide outputs, else 8
static int x3_gn_th(int cout_p) { return cout_p == 64 ? 12 : 8; }
// split-bf16 (IC2_BF16X3) / split-weight f16 (IC2_F16X2) conv with f32 output: the hg4 instance the plan picks (per
// chunk of *nc images, as ic2_conv_igemm_ws launches it) carries the statistics in its epilogue when it is a
// 32-wide-tile o64 / o128 kernel over exactly 32 groups of 2 / 4 channels.  *plan: that instance on the statistics
// kernel's tile rows
static bool x3_gn_hg4(int dtype, int n, int h, int w_, int cin_p, int cout_p, int cout_valid, int kh, int kw, int pad,
                      int groups, H4Plan* plan = nullptr, int* nc = nullptr) {
  const int ho = h + 2 * pad - kh + 1, wo = w_ + 2 * pad - kw + 1;
  if (ho <= 0 || wo <= 0 || groups != 32 || cout_valid != cout_p || (cout_p != 64 && cout_p != 128)) return false;
  int nc_;
  const ConvPlan c = conv_choice_chunked(dtype, IC2_LAYOUT_NHWC, IC2_F32, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, &nc_);
  if (c.kind != CK_HG4 || !c.h4.tw32 || c.h4.bo != cout_p) return false;
  if (plan) *plan = c.h4, plan->th = x3_gn_th(cout_p);
  if (nc) *nc = nc_;
  return true;
}
static int64_t x3_gn_tiles(int ho, int wo, int cout_p) { return ceil_div(wo, 32) * ceil_div(ho, x3_gn_th(cout_p)); }
// on unless refused (fuse_mode 0): the statistics epilogue of the non-persistent hg4 costs less than the separate f32
// pass saves
static bool x3_gn_requested(int fuse_mode) { return fuse_mode != 0; }
static bool x3_dtype(int dtype) { return dtype == IC2_BF16X3 || dtype == IC2_F16X2; }

bool conv_gn_fuses(int dtype, int n, int h, int w_, int cin_p, int cout_p, int cout_valid, int kh, int kw, int pad,
                   int groups, int fuse_mode) {
  return x3_dtype(dtype) && x3_gn_requested(fuse_mode) &&
         x3_gn_hg4(dtype, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, groups);
}

int conv_gn_fused(const void* x, const void* w, void* y, int dtype, int n, int h, int w_, int cin_p, int cout_p,
                  int cout_valid, int kh, int kw, int pad, const float* bias, int groups, double* part,
                  int64_t part_doubles, void* workspace, int64_t ws_bytes, int fuse_mode, hipStream_t s, float out_mul) {
  const int ho = h + 2 * pad - kh + 1, wo = w_ + 2 * pad - kw + 1;
  // Output of the split modes: f32 (split bf16) / f16 (split-weight f16: its consumer's operand is f16 anyway)
  const int ydt = dtype == IC2_F16X2 ? IC2_F16 : dtype == IC2_BF16X3 ? IC2_F32 : dtype;
  H4Plan p;
  int nc = n;
  const int64_t ntile = x3_gn_tiles(ho, wo, cout_p);  // the statistics kernel's 32-wide tiles per image
  const bool fuse = x3_dtype(dtype) && x3_gn_requested(fuse_mode) && bias != nullptr && part != nullptr &&
                    part_doubles >= (int64_t)n * groups * ntile * 2 &&
                    x3_gn_hg4(dtype, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, groups, &p, &nc);
  if (!fuse) {
    const int rc = ic2_conv_igemm_ws(x, w, y, dtype, ydt, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, ho, wo,
                                     nullptr, bias, 0, 0.f, 1.f, -1.f, out_mul, IC2_LAYOUT_NHWC, workspace, ws_bytes, s);
    return rc == IC2_OK ? 0 : -1;
  }
  IgemmArgs a = make_igemm_args(x, w, y, bias, dtype, ydt, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, out_mul);
  a.gn_groups = groups; a.gn_c = cout_valid;
  for (int i0 = 0; i0 < n; i0 += nc) {  // chunks of whole images (< 2^31 input bytes per launch)
    const int cnt = n - i0 < nc ? n - i0 : nc;
    a.x = reinterpret_cast<const char*>(x) + (int64_t)i0 * h * w_ * a.x_pix * 2;
    a.y = reinterpret_cast<char*>(y) + (int64_t)i0 * ho * wo * cout_p * (ydt == IC2_F16 ? 2 : 4);
    a.gn_part = part + (int64_t)i0 * groups * ntile * 2;
    a.n = cnt;
    a.M = (int)((int64_t)cnt * ho * wo);
    launch_hg4(a, p, dtype == IC2_F16X2, true, s);
  }
  return (int)ntile;
}

int64_t conv_gn_fused_part_doubles(int dtype, int n, int h, int w_, int cin_p, int cout_p, int kh, int kw, int pad,
                                   int groups) {
  const int ho = h + 2 * pad - kh + 1, wo = w_ + 2 * pad - kw + 1;
  return x3_dtype(dtype) && x3_gn_hg4(dtype, n, h, w_, cin_p, cout_p, cout_p, kh, kw, pad, groups)
             ? (int64_t)n * groups * x3_gn_tiles(ho, wo, cout_p) * 2 : 0;
}
}  // namespace ic2
