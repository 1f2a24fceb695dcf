// Fused filtered leaky-ReLU with a NON-SEPARABLE (2-D) down filter: the StyleGAN3-R configuration, whose non-critical
// layers low-pass with a radially symmetric 12 x 12 filter [SG3-public: training/networks_stylegan3.py
// design_lowpass_filter(radial=True); torch_utils/ops/filtered_lrelu.py reference path
//   bias_act(b) -> upfirdn2d(fu, up, padding, gain=up^2) -> bias_act(lrelu, slope, gain, clamp) -> upfirdn2d(fd2d, down)].
// The up filter stays separable (SG3-R designs only the down filters radially).
//
// One workgroup = one (sample, TOY x TOX output tile, 16-channel block); lanes own channel pairs and accumulate in f32.
// The activated up-sampled tile lives only in LDS (f32 pairs on the f32 path, f16 pairs on the 16-bit paths):
//   stage 1  vertical up-FIR   : input column (registers) -> LDS row i, columns 0 .. NINX-1
//   stage 2  horizontal up-FIR : LDS row (registers) -> lrelu, clamp -> written back over the thread's own row, even and
//                                odd grid columns in separate planes (stage 3 then reads consecutive addresses)
//   stage 3  all 12 x 12 down taps per output, RY output rows of one column per lane -> * post_scale -> global
// The polyphase up-FIR (up_fir), the pair access, the LDS packing, the activation and the host helpers are
// flrelu_valu.h's, shared with flrelu.hip; the zero padding / crop is handled as there.  Input NHWC or channel-blocked
// NHWC16, output NHWC or NHWC16: the layouts differ in strides only, so they give the same bits.
#include "flrelu.h"
#include "flrelu_valu.h"

namespace ic2 {
namespace {

constexpr int R2_D = 2, R2_TD = 12;  // the instances: down 2 with a 12 x 12 filter
constexpr int R2_NCG = 8;            // channel pairs per workgroup (16 channels)
constexpr int R2_THREADS = 256;
constexpr int R2_MAX_RANK = 4;

struct Flr2dArgs {
  const void* x;
  void* y;
  const float* bias;
  const float* post_scale;      // [n][c_p] or null
  int64_t xsn, xsy, xsx, xcb;   // input strides (elements); channels of a 16-block are contiguous, xcb = next block
  int64_t ysn, ysy, ysx, ycb;   // output strides
  int c_p, in_h, in_w, out_h, out_w;
  int py0, px0;
  int tiles_x, tiles_y, cblocks;
  float slope, lim;             // lrelu slope (<= 1), clamp bound / gain (finite on the f16-LDS paths)
  float gu[24];                 // up taps, flipped unless flip_filter, times up
  float gd[R2_TD * R2_TD];      // down taps [tx][ty] (transposed: stage 3 walks ty), flipped unless flip_filter, times gain
};

template <int U, int TU, int TOY, int TOX> struct R2Geom {
  static constexpr int RAY = (TOY - 1) * R2_D + R2_TD;  // activated-grid rows / columns of one tile
  static constexpr int RAX = (TOX - 1) * R2_D + R2_TD;
  static constexpr int NINY = (RAY + TU - 2) / U + 1;   // input rows / columns feeding them
  static constexpr int NINX = (RAX + TU - 2) / U + 1;
  static constexpr int PH = RAX / 2;                    // columns per parity plane
  static constexpr int ROW = (2 * PH + 1) * R2_NCG;     // row pitch in pairs: one pad column keeps 4 rows on 32 banks
  static_assert(RAX % 2 == 0 && NINX <= 2 * PH, "the up-sampled row must fit the activated row it is replaced by");
  static_assert((TOY * R2_D) % U == 0 && (TOX * R2_D) % U == 0, "tile origins must keep the polyphase offset");
};

template <typename TI, typename TO, int U, int TU, int DELTA, int TOY, int TOX, int RY>
__global__ void __launch_bounds__(R2_THREADS) flrelu_radial_kernel(Flr2dArgs a) {
  static_assert(TU % U == 0 && TOY % RY == 0, "whole polyphase phases, whole row groups");
  using G = R2Geom<U, TU, TOY, TOX>;
  using LT = typename std::conditional<std::is_same<TI, float>::value, f2v, h2v>::type;
  using LP = LdsPair<LT>;
  constexpr int RAY = G::RAY, RAX = G::RAX, NINY = G::NINY, NINX = G::NINX, PH = G::PH, ROW = G::ROW;
  constexpr int NCG = R2_NCG, D = R2_D, TD = R2_TD;
  __shared__ __attribute__((aligned(16))) LT buf[RAY * ROW];
  // the 144 down taps: read from LDS by a run-time tap column in stage 3 (in SGPRs they spill: every index there is
  // a compile-time constant, so the compiler loads all of them up front)
  __shared__ __attribute__((aligned(16))) float taps[TD * TD];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int t = 0; t < TD * TD; ++t) taps[t] = a.gd[t];
  }

  const FlrBlock blk = flr_block(a);
  const int cb = blk.cb, tx = blk.tx, ty = blk.ty, n = blk.n;

  const int oy0 = ty * TOY, ox0 = tx * TOX;
  const int sy0 = (oy0 * D - a.py0 + DELTA) / U;  // exact: DELTA == p0 (mod U) and U divides the tile origin * D
  const int sx0 = (ox0 * D - a.px0 + DELTA) / U;

  const TI* __restrict__ xin = reinterpret_cast<const TI*>(a.x) + (int64_t)n * a.xsn + (int64_t)cb * a.xcb;
  TO* __restrict__ yout = reinterpret_cast<TO*>(a.y) + (int64_t)n * a.ysn + (int64_t)cb * a.ycb;

  // ---------------- stage 1: vertical up-FIR of NINX input columns
  for (int item = threadIdx.x; item < NINX * NCG; item += R2_THREADS) {
    const int xs = item / NCG;
    const int cg = item - xs * NCG;
    const int ix = sx0 + xs;
    const bool col_ok = (unsigned)ix < (unsigned)a.in_w;
    f2v bsum = f2v{0.f, 0.f};
    if (a.bias) bsum = f2v{a.bias[cb * 16 + 2 * cg], a.bias[cb * 16 + 2 * cg + 1]};
    const TI* pcol = xin + (int64_t)ix * a.xsx + 2 * cg;
    f2v in[NINY];
#pragma unroll
    for (int j = 0; j < NINY; ++j) {
      const int iy = sy0 + j;
      const bool ok = col_ok && (unsigned)iy < (unsigned)a.in_h;
      const f2v v = load_pair<TI>(pcol + (int64_t)iy * a.xsy, ok) + bsum;
      in[j] = ok ? v : f2v{0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < RAY; ++i) buf[i * ROW + xs * NCG + cg] = LP::pack(up_fir<U, TU, DELTA, NINY>(a.gu, i, in));
  }
  __syncthreads();

  // ---------------- stage 2: horizontal up-FIR and activation per grid row; column k goes to plane k & 1
  for (int item = threadIdx.x; item < RAY * NCG; item += R2_THREADS) {
    const int i = item / NCG;
    const int cg = item - i * NCG;
    f2v in[NINX];
#pragma unroll
    for (int j = 0; j < NINX; ++j) in[j] = LP::unpack(buf[i * ROW + j * NCG + cg]);
#pragma unroll
    for (int k = 0; k < RAX; ++k)
      buf[i * ROW + ((k & 1) * PH + (k >> 1)) * NCG + cg] =
          LP::pack(act2(up_fir<U, TU, DELTA, NINX>(a.gu, k, in), a.slope, a.lim));
  }
  __syncthreads();

  // ---------------- stage 3: the 2-D down FIR; a lane owns RY output rows of one column and one channel pair
  constexpr int RGI = (RY - 1) * D + TD;  // grid rows feeding RY output rows
  for (int item = threadIdx.x; item < NCG * TOX * (TOY / RY); item += R2_THREADS) {
    const int cg = item % NCG;
    const int ox = (item / NCG) % TOX;
    const int rg = item / (NCG * TOX);
    const int gx = ox0 + ox;
    if (gx >= a.out_w) continue;
    f2v o[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) o[r] = f2v{0.f, 0.f};
    const LT* prow = buf + rg * RY * D * ROW + cg;
#pragma unroll 1
    for (int t = 0; t < TD; ++t) {  // tap column: grid column ox * D + t = plane t & 1, index ox + t / 2
      float g[TD];
#pragma unroll
      for (int u = 0; u < TD; ++u) g[u] = taps[t * TD + u];
      const LT* pc = prow + ((t & 1) * PH + ox + (t >> 1)) * NCG;
#pragma unroll
      for (int ii = 0; ii < RGI; ++ii) {
        const f2v v = LP::unpack(pc[ii * ROW]);
#pragma unroll
        for (int m = 0; m < TD / D; ++m) {
          const int r = ii / D - m;
          if (r >= 0 && r < RY) o[r] += g[ii - r * D] * v;
        }
      }
    }
    f2v ps = f2v{1.f, 1.f};
    if (a.post_scale) {
      const float* pp = a.post_scale + (int64_t)n * a.c_p + cb * 16 + 2 * cg;
      ps = f2v{pp[0], pp[1]};
    }
    TO* pout = yout + (int64_t)gx * a.ysx + 2 * cg;
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      const int gy = oy0 + rg * RY + r;
      if (gy < a.out_h) store_pair_fwd<TO>(pout + (int64_t)gy * a.ysy, o[r] * ps);
    }
  }
}

// Tiles: 16 x 16 outputs on the 16-bit paths (f16 LDS, 56.4 KiB), 8 x 8 in f32 (44.3 KiB)
template <typename TI> struct R2Tile {
  static constexpr int TOY = 16, TOX = 16, RY = 8;
};
template <> struct R2Tile<float> {
  static constexpr int TOY = 8, TOX = 8, RY = 2;
};

template <typename TI, typename TO, int U, int TU, int DL>
int launch_geom(Flr2dArgs& a, int n, hipStream_t s) {
  using T = R2Tile<TI>;
  a.tiles_x = (int)ceil_div(a.out_w, T::TOX);
  a.tiles_y = (int)ceil_div(a.out_h, T::TOY);
  a.cblocks = a.c_p / 16;
  const int64_t grid = (int64_t)n * a.tiles_y * a.tiles_x * a.cblocks;
  if (grid >= (1LL << 31)) {
    set_error("flrelu_nhwc_2d: grid too large");
    return IC2_E_INVALID;
  }
  hipLaunchKernelGGL((flrelu_radial_kernel<TI, TO, U, TU, DL, T::TOY, T::TOX, T::RY>), dim3((unsigned)grid),
                     dim3(R2_THREADS), 0, s, a);
  return IC2_OK;
}

template <typename TI, typename TO>
int launch_cfg(Flr2dArgs& a, int up, int delta, int n, hipStream_t s) {
  if (up == 2) {
    switch (delta) {
      case 0: return launch_geom<TI, TO, 2, 12, 0>(a, n, s);
      case 1: return launch_geom<TI, TO, 2, 12, 1>(a, n, s);
    }
  } else if (up == 4) {
    switch (delta) {
      case 0: return launch_geom<TI, TO, 4, 24, 0>(a, n, s);
      case 1: return launch_geom<TI, TO, 4, 24, 1>(a, n, s);
      case 2: return launch_geom<TI, TO, 4, 24, 2>(a, n, s);
      case 3: return launch_geom<TI, TO, 4, 24, 3>(a, n, s);
    }
  }
  return IC2_E_UNSUPPORTED;
}

int flrelu_2d_common(const void* x, void* y, int dtype_in, int dtype_out, bool in_blocked, int n, int c_p, int in_h,
                     int in_w, int out_h, int out_w, const float* fu, int fu_taps, const float* fd, int fd_taps,
                     int rank, const float* fd_v, const float* fd_h, const float* b, int up, int down, int px0, int px1,
                     int py0, int py1, float gain, float slope, float clamp, int flip, const float* post_scale,
                     void* stream, const char* name) {
  IC2_CHECK_ARG(x && y && fu && fd, "%s: null pointer", name);
  const int out_layout = IC2_FLR_OUT_LAYOUT_OF(dtype_out);
  dtype_out = IC2_FLR_DTYPE_OF(dtype_out);
  IC2_CHECK_ARG(out_layout == IC2_LAYOUT_NHWC || out_layout == IC2_LAYOUT_NHWC16, "%s: output layout %d (NHWC or NHWC16)",
                name, out_layout);
  const bool out_blocked = out_layout == IC2_LAYOUT_NHWC16;
  IC2_CHECK_ARG(n > 0 && c_p > 0 && c_p % 16 == 0 && in_h > 0 && in_w > 0 && up >= 1 && down >= 1,
                "%s: bad geometry (c_p a multiple of 16)", name);
  IC2_CHECK_ARG(fu_taps >= 1 && fu_taps <= 24 && fd_taps >= 1 && fd_taps <= R2_TD,
                "%s: unsupported taps %d / %d x %d (at most 24 / 12 x 12)", name, fu_taps, fd_taps, fd_taps);
  IC2_CHECK_ARG(rank >= 0 && rank <= R2_MAX_RANK, "%s: rank %d (0 = direct, at most %d)", name, rank, R2_MAX_RANK);
  IC2_CHECK_ARG(rank == 0 || (fd_v && fd_h), "%s: rank %d without its tap vectors", name, rank);
  const int64_t ew = flr_out_size(in_w, up, px0, px1, fu_taps, fd_taps, down);
  const int64_t eh = flr_out_size(in_h, up, py0, py1, fu_taps, fd_taps, down);
  IC2_CHECK_ARG(out_h == eh && out_w == ew, "%s: output %dx%d, expected %lldx%lld", name, out_h, out_w, (long long)eh,
                (long long)ew);
  IC2_CHECK_ARG(out_h > 0 && out_w > 0, "%s: empty output", name);
  const bool p32 = dtype_in == IC2_F32 && dtype_out == IC2_F32;
  const bool p16 = (dtype_in == IC2_F16 && (dtype_out == IC2_F16 || dtype_out == IC2_BF16)) ||
                   (dtype_in == IC2_BF16 && dtype_out == IC2_BF16);
  IC2_CHECK_ARG(p32 || p16, "%s: unsupported dtype pair %d -> %d", name, dtype_in, dtype_out);
  IC2_CHECK_ARG(p16 || (!in_blocked && !out_blocked), "%s: the channel-blocked layouts are 16-bit", name);
  const int dx = ((px0 % up) + up) % up, dy = ((py0 % up) + up) % up;
  if (dx != dy) {  // one polyphase offset serves both axes
    set_error("%s: px0 and py0 differ mod up", name);
    return IC2_E_UNSUPPORTED;
  }
  if (!flr_act_ok(slope, gain)) {
    set_error("%s: fused path needs 0 <= slope <= 1 and gain > 0", name);
    return IC2_E_UNSUPPORTED;
  }
  if (!((up == 2 || up == 4) && fu_taps == 6 * up && down == R2_D && fd_taps == R2_TD)) {
    set_error("%s: no fused instance for up=%d down=%d taps=%d / %dx%d (up 2/4 with 6*up taps, down 2 with 12x12)", name,
              up, down, fu_taps, fd_taps, fd_taps);
    return IC2_E_UNSUPPORTED;
  }
  Flr2dArgs a;
  a.x = x; a.y = y; a.bias = b; a.post_scale = post_scale;
  const int64_t c = c_p;
  if (in_blocked) {  // [n][c_p / 16][in_h][in_w][16]
    a.xsx = 16; a.xsy = (int64_t)in_w * 16; a.xcb = (int64_t)in_h * in_w * 16;
  } else {
    a.xsx = c; a.xsy = (int64_t)in_w * c; a.xcb = 16;
  }
  a.xsn = (int64_t)in_h * in_w * c;
  if (out_blocked) {
    a.ysx = 16; a.ysy = (int64_t)out_w * 16; a.ycb = (int64_t)out_h * out_w * 16;
  } else {
    a.ysx = c; a.ysy = (int64_t)out_w * c; a.ycb = 16;
  }
  a.ysn = (int64_t)out_h * out_w * c;
  a.c_p = c_p;
  a.in_h = in_h; a.in_w = in_w; a.out_h = out_h; a.out_w = out_w;
  a.py0 = py0; a.px0 = px0;
  a.tiles_x = a.tiles_y = a.cblocks = 0;
  a.slope = slope;
  // the gain rides on the down taps, the clamp bound is divided by it; the f16 LDS tile holds at most the f16 range
  a.lim = flr_lim(clamp, gain);
  if (p16 && !(a.lim < 65504.f)) a.lim = 65504.f;
  flr_up_taps(a.gu, fu, fu_taps, up, flip);
  for (int ty = 0; ty < R2_TD; ++ty)
    for (int tx = 0; tx < R2_TD; ++tx)
      a.gd[tx * R2_TD + ty] = (flip ? fd[ty * R2_TD + tx] : fd[(R2_TD - 1 - ty) * R2_TD + (R2_TD - 1 - tx)]) * gain;
  // rank > 0 offers a separable factorisation; this build has no low-rank instance, so every call takes the direct
  // kernel on fd itself (StyleGAN3-R)
  (void)fd_v; (void)fd_h;
  hipStream_t s = as_stream(stream);
  int rc;
  if (p32) rc = launch_cfg<float, float>(a, up, dx, n, s);
  else if (dtype_in == IC2_BF16) rc = launch_cfg<bf16_t, bf16_t>(a, up, dx, n, s);
  else if (dtype_out == IC2_F16) rc = launch_cfg<_Float16, _Float16>(a, up, dx, n, s);
  else rc = launch_cfg<_Float16, bf16_t>(a, up, dx, n, s);
  if (rc != IC2_OK) return rc;
  IC2_CHECK_LAUNCH(name);
  return IC2_OK;
}

}  // namespace
}  // namespace ic2

using namespace ic2;

extern "C" int ic2_flrelu_nhwc_2d(const void* x, void* y, int dtype_in, int dtype_out, int n, int c_p, int in_h,
                                  int in_w, int out_h, int out_w, const float* fu, int fu_taps, const float* fd,
                                  int fd_taps, int rank, const float* fd_v, const float* fd_h, const float* b, int up,
                                  int down, int px0, int px1, int py0, int py1, float gain, float slope, float clamp,
                                  int flip, const float* post_scale, void* stream) {
  return flrelu_2d_common(x, y, dtype_in, dtype_out, false, n, c_p, in_h, in_w, out_h, out_w, fu, fu_taps, fd, fd_taps,
                          rank, fd_v, fd_h, b, up, down, px0, px1, py0, py1, gain, slope, clamp, flip, post_scale,
                          stream, "flrelu_nhwc_2d");
}

extern "C" int ic2_flrelu_nhwc16_2d(const void* x, void* y, int dtype_in, int dtype_out, int n, int c_p, int in_h,
                                    int in_w, int out_h, int out_w, const float* fu, int fu_taps, const float* fd,
                                    int fd_taps, int rank, const float* fd_v, const float* fd_h, const float* b, int up,
                                    int down, int px0, int px1, int py0, int py1, float gain, float slope, float clamp,
                                    int flip, const float* post_scale, void* stream) {
  return flrelu_2d_common(x, y, dtype_in, dtype_out, true, n, c_p, in_h, in_w, out_h, out_w, fu, fu_taps, fd, fd_taps,
                          rank, fd_v, fd_h, b, up, down, px0, px1, py0, py1, gain, slope, clamp, flip, post_scale,
                          stream, "flrelu_nhwc16_2d");
}
