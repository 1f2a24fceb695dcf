// Host side of the conv kernels: the launch plan (computed once per call by conv_choice, conv_dispatch.hip, and read by
// the launch, the plan-name query and the workspace query alike), each kernel family's launcher and the fused
// conv + GroupNorm entry points encoder_ops.hip calls.
#pragma once
#include "conv_common.h"

namespace ic2 {

// implicit-GEMM tile instances; IC2_IGEMM_TILE=1..7 (IC2_DEV=1) forces a 2-byte one by id
enum IgTileId {
  IG_F32_128x128 = 0,  // exact-f32 MFMA, 2-stage ring
  IG_256x256 = 1, IG_32x256 = 2, IG_128x256 = 3, IG_128x128 = 4, IG_64x256 = 5,  // 4-stage ring (igemm.hip)
  IG_G8_OG2 = 6, IG_G8_OG1 = 7,                                                  // 8-phase (igemm8.hip)
};
struct IgTile {
  int id, bo, bp;
  const char* name;  // plan-name stem
};
constexpr IgTile kIgTiles[8] = {
    {IG_F32_128x128, 128, 128, "igemm_f32_128x128"}, {IG_256x256, 256, 256, "igemm_256x256"},
    {IG_32x256, 32, 256, "igemm_32x256"},            {IG_128x256, 128, 256, "igemm_128x256"},
    {IG_128x128, 128, 128, "igemm_128x128"},         {IG_64x256, 64, 256, "igemm_64x256"},
    {IG_G8_OG2, 256, 256, "igemm8_og2"},             {IG_G8_OG1, 128, 512, "igemm8_og1"}};

// hg4 instance: o-tile bo on th x tw-pixel tiles (tw32: 32-wide, else 16-wide); area = a sample's output padded to
// whole tiles, blocks = workgroups of the launch
struct H4Plan {
  int bo;
  bool tw32;
  int th, tw;
  int64_t area, blocks;
};

enum ConvKind { CK_TORGB, CK_HG4, CK_HCONV, CK_IGEMM };
struct ConvPlan {
  ConvKind kind;
  // CK_IGEMM: tile instance, K slices (gridDim.y), and the two-launch forms of the 8-phase tiles
  int tile, splits;
  bool tail;      // IG_G8_OG2: whole rounds at full K, then the tiles from tail_tile on (pixels from p_lo) split over K in two
  bool split384;  // IG_G8_OG1 on an odd multiple of 128 above 128: og2 on all but the last 128 channels, og1 on those
  int tail_tile, p_lo;
  int64_t ws_bytes;  // f32 partial sums of the split forms (0: none)
  H4Plan h4;         // CK_HG4
  int hc_cin, hc_cout;  // CK_HCONV: the instance's channel counts
};

// launchers, one per kernel family, each next to its kernels
void launch_igemm(const IgemmArgs& a, int tile, bool f16, int splits, hipStream_t s);               // igemm.hip
void launch_splitk_reduce(const IgemmArgs& a, int splits, int p_lo, hipStream_t s);                 // igemm.hip
void launch_igemm8(const IgemmArgs& a, const ConvPlan& c, bool f16, hipStream_t s);                 // igemm8.hip
void launch_hg4(IgemmArgs a, const H4Plan& p, bool f16, bool gn_stats, hipStream_t s);              // hg4.hip
void launch_hconv(const IgemmArgs& a, bool f16, hipStream_t s);                                     // hconv.hip
void launch_torgb(const IgemmArgs& a, bool f16, hipStream_t s);                                     // hconv.hip

// conv_dispatch.hip: what the two conv entry points (ic2_conv_igemm_ws, ic2_conv_wino in wino.hip) share.  A ConvCall
// is the entry point's arguments; conv_check_call runs the checks both make (error texts under the entry's name `who`)
// and decodes the input-layout bits of `act` and the IEEE flavour of an f16 output; conv_for_chunks then hands `launch`
// the launch arguments of each chunk of whole images (conv_chunk_n), all of them in one chunk as a rule.
struct ConvCall {
  const void *x, *w;
  void* y;
  const float *oscale, *bias;
  int dtype, out_dtype, n, h, w_, cin_p, cout_p, cout_valid, kh, kw, pad, ho, wo;
  int act;  // as passed: IC2_ACT_IN_LAYOUT bits above the activation; the activation alone after conv_check_call
  float slope, act_gain, clamp, out_mul;
  int out_layout;
  bool in_blocked;  // set by conv_check_call: channel-blocked (NHWC16) input
  int out_ieee;     // set by conv_check_call: out_dtype was IC2_F16_IEEE (out_dtype becomes IC2_F16)
};
int conv_check_call(const char* who, ConvCall& c);
int conv_chunk_n(int dtype, int n, int h, int w_, int cin_p);
int64_t conv_x_img_bytes(int dtype, int h, int w_, int cin_p);
IgemmArgs make_igemm_args(const void* x, const void* w, void* y, const float* bias, int dtype, int out_dtype, int n,
                          int h, int w_, int cin_p, int cout_p, int cout_valid, int kh, int kw, int pad, float out_mul);
template <class Launch>
int conv_for_chunks(const ConvCall& c, Launch&& launch) {
  const int nc = conv_chunk_n(c.dtype, c.n, c.h, c.w_, c.cin_p);
  const int64_t x_img = conv_x_img_bytes(c.dtype, c.h, c.w_, c.cin_p);
  const int64_t y_img = c.out_layout == IC2_LAYOUT_NCHW
                            ? (int64_t)c.cout_valid * c.ho * c.wo * 4
                            : (int64_t)c.ho * c.wo * c.cout_p * (c.out_dtype == IC2_F32 ? 4 : 2);
  for (int n0 = 0; n0 < c.n; n0 += nc) {
    IgemmArgs a = make_igemm_args(reinterpret_cast<const char*>(c.x) + n0 * x_img, c.w,
                                  reinterpret_cast<char*>(c.y) + n0 * y_img, c.bias, c.dtype, c.out_dtype,
                                  c.n - n0 < nc ? c.n - n0 : nc, c.h, c.w_, c.cin_p, c.cout_p, c.cout_valid, c.kh, c.kw,
                                  c.pad, c.out_mul);
    a.oscale = c.oscale ? c.oscale + (int64_t)n0 * c.cout_p : nullptr;
    a.act = c.act; a.slope = c.slope; a.act_gain = c.act_gain; a.clamp = c.clamp;
    a.out_layout = c.out_layout; a.out_ieee = c.out_ieee;
    ig_set_input_layout(a, c.in_blocked);
    const int rc = launch(a);
    if (rc != IC2_OK) return rc;
  }
  return IC2_OK;
}

// conv_dispatch.hip: conv (bias only, NHWC out) with the GroupNorm partial sums fused into the hg4 kernels' epilogue
// when the plan picks one that carries them (the split modes only).  conv_gn_fused returns the number of per-image
// tiles written to `part` ([n][groups][tiles][2] f64), 0 when the conv ran unfused (the caller then computes the
// statistics itself) and -1 on an argument error (message set).  fuse_mode: 0 = never fuse, else the plan's choice.
int conv_gn_fused(const void* x, const void* w, void* y, int dtype, int n, int h, int w_, int cin_p, int cout_p,
                  int cout_valid, int kh, int kw, int pad, const float* bias, int groups, double* part,
                  int64_t part_doubles, void* workspace, int64_t ws_bytes, int fuse_mode, hipStream_t s,
                  float out_mul = 1.f);
bool conv_gn_fuses(int dtype, int n, int h, int w_, int cin_p, int cout_p, int cout_valid, int kh, int kw, int pad,
                   int groups, int fuse_mode);
int64_t conv_gn_fused_part_doubles(int dtype, int n, int h, int w_, int cin_p, int cout_p, int kh, int kw, int pad,
                                   int groups);

}  // namespace ic2
