// Backward of the fused filtered leaky-ReLU with a 2-D (radial, non-separable) down filter on NHWC activations:
// the gradient of ic2_flrelu_nhwc_2d (flrelu_radial.hip) w.r.t. its input, for training an encoder through a frozen
// StyleGAN3-R generator.  Contract and notation of flrelu_bwd.hip (its header comment), with the down filter 2-D:
//   gd2[ty][tx] = fd[td-1-ty][td-1-tx] (upfirdn2d: flipped in both axes unless `flip`, gain 1; row = y)
//   gV[ky][kx] = sum_{oy,ox} gd2[ky - 2*oy][kx - 2*ox] * gout[oy][ox]      polyphase adjoint: 6 x 6 live taps
//   gU = gV * gain * (U > 0 ? 1 : slope) * (|gain * lrelu(U)| < clamp)     U recomputed from x, separable up FIR
//   gx[i] = separable adjoint up FIR of gU;  stored gx * oscale[n][c];  ydot = per-tile sums of gx * (x - bias)
// One workgroup = one (sample, TIY x TIX tile of gx, NP channel pairs), f32 arithmetic and f32 LDS throughout:
//   stage A  x columns -> vertical up-FIR rows of U (LDS a_v); the gout tile with its halo, raw (LDS g_s); the
//            taps (LDS: stage B indexes them at run time -- compile-time indices of 144 kernel-argument taps all
//            land in SGPRs and spill, and stage B's index is per lane)
//   stage B  per grid position, strips of 4 same-parity columns: horizontal up-FIR (U), the 36-tap gather (gV) on
//            a 6 x 9 gout window, gU = gV * act'(U) -> LDS b_v
//   stage B2 per grid row: horizontal down-by-up FIR of gU, written over the row's a_v
//   stage C  per column: vertical down-by-up FIR -> gx (f32) -> global, ydot partials
// With R >= 10 and down 2 every one of the 36 gather taps of every grid position of the tile is inside the staged
// window (oy = (R + k) / 2 - m >= 0 for m < 6), so the gather has no bounds tests.
// Stage A's up-FIR rows, stage B2's scatter and all of stage C are flrelu_valu.h's (bwd_up_rows, up_adjoint,
// bwd_stage_c), shared with flrelu_bwd.hip; this file's store is the gradient store of its TO (f16 converted IEEE).
#include "flrelu_valu.h"

namespace ic2 {

constexpr int RB_TD = 12;   // down taps per axis
constexpr int RB_DN = 2;

struct FlrRadBwdArgs {
  const void* x;        // conv output that fed the forward (NHWC [n][in_h][in_w][c_p], f32 or f16)
  const void* gout;     // gradient of the layer output (NHWC [n][out_h][out_w][c_p])
  void* gx;             // gradient of x (NHWC), times oscale[n][c] when oscale is set
  const float* oscale;  // [n][c_p] or null
  const float* bias;    // [c_p] or null
  float* ydot;          // [n][tiles][c_p] or null
  int c_p;
  int in_h, in_w, out_h, out_w;
  int p0;
  int tiles_x, tiles_y, cblocks;
  float slope, gain, lim;  // lim = clamp / gain (+inf: no clamp)
  float gu[24];            // up taps, flipped unless flip, times up
  float gd[RB_TD * RB_TD];  // gd2 [ty][tx], flipped unless flip
};

template <typename TI, typename TG, typename TO, int UP, int TU, int R, int TIY, int TIX, int NP, int NT>
__global__ void __launch_bounds__(NT) flrelu_radial_bwd_kernel(FlrRadBwdArgs a) {
  static_assert(TU == 6 * UP && UP % RB_DN == 0 && R >= RB_TD - 2 && R < RB_TD, "polyphase loops assume whole phases");
  constexpr int DN = RB_DN, TD = RB_TD;
  constexpr int KY = (TIY - 1) * UP + TU;  // lrelu-grid rows / columns feeding the tile
  constexpr int KX = (TIX - 1) * UP + TU;
  constexpr int NJY = TIY + 2 * (TU / UP) - 2;  // x rows / columns feeding them
  constexpr int NJX = TIX + 2 * (TU / UP) - 2;
  constexpr int NOY = (R + KY - 1) / DN + 1;  // gout rows / columns feeding the grid rows
  constexpr int NOX = (R + KX - 1) / DN + 1;
  constexpr int PA = NJX | 1, PB = KX | 1, PG = NOX | 1;  // odd row pitches
  constexpr int SW = 4;                                    // same-parity columns per stage-B strip
  constexpr int NS = ((KX + 1) / 2 + SW - 1) / SW;         // strips per column parity
  static_assert(TIX <= NJX, "stage B2 writes its TIX results over the row's a_v");
  __shared__ __attribute__((aligned(16))) f2v a_v[KY * PA * NP];
  __shared__ __attribute__((aligned(16))) f2v b_v[KY * PB * NP];
  __shared__ __attribute__((aligned(16))) f2v g_s[NOY * PG * NP];
  __shared__ float s_gd[TD * TD];
  __shared__ float s_gu[TU];
  static_assert(sizeof(f2v) * (KY * PA + KY * PB + NOY * PG) * NP + 4 * (TD * TD + TU) <= 64 * 1024,
                "two workgroups per CU");

  const FlrBlock blk = flr_block(a);
  const int cb = blk.cb, tx = blk.tx, ty = blk.ty, n = blk.n;
  const int i0y = ty * TIY, i0x = tx * TIX;
  const int j0y = i0y - TU / UP + 1, j0x = i0x - TU / UP + 1;
  // first gout row / column: (k0 - td + 1 + ph) / down, exact (R = td - 1 - ph)
  const int o0y = (i0y * UP + a.p0 - TU + 1 - R) / DN;
  const int o0x = (i0x * UP + a.p0 - TU + 1 - R) / DN;
  const int c0 = cb * 2 * NP;
  const TI* __restrict__ xin = reinterpret_cast<const TI*>(a.x) + (int64_t)n * a.in_h * a.in_w * a.c_p;
  const TG* __restrict__ gin = reinterpret_cast<const TG*>(a.gout) + (int64_t)n * a.out_h * a.out_w * a.c_p;

  // ---------------- stage A: taps, the gout window, the vertical up pass of x
  for (int t = threadIdx.x; t < TD * TD; t += NT) s_gd[t] = a.gd[t];
  if (threadIdx.x < TU) s_gu[threadIdx.x] = a.gu[threadIdx.x];
  for (int item = threadIdx.x; item < NOY * NOX * NP; item += NT) {
    const int p = item % NP;
    const int oc = (item / NP) % NOX;
    const int orow = item / (NP * NOX);
    const int oy = o0y + orow, ox = o0x + oc;
    const bool ok = (unsigned)oy < (unsigned)a.out_h && (unsigned)ox < (unsigned)a.out_w;
    const f2v v = load_pair<TG>(gin + ((int64_t)oy * a.out_w + ox) * a.c_p + c0 + 2 * p, ok);
    g_s[(orow * PG + oc) * NP + p] = ok ? v : f2v{0.f, 0.f};
  }
  for (int item = threadIdx.x; item < NJX * NP; item += NT) {
    const int col = item / NP;
    const int p = item - col * NP;
    const int ix = j0x + col;
    const bool cok = (unsigned)ix < (unsigned)a.in_w;
    const TI* pc = xin + (int64_t)ix * a.c_p + c0 + 2 * p;
    f2v in[NJY];
#pragma unroll
    for (int j = 0; j < NJY; ++j) {
      const int iy = j0y + j;
      const bool ok = cok && (unsigned)iy < (unsigned)a.in_h;
      const f2v v = load_pair<TI>(pc + (int64_t)iy * a.in_w * a.c_p, ok);
      in[j] = ok ? v : f2v{0.f, 0.f};
    }
    bwd_up_rows<UP, TU, KY, NJY>(a.gu, in, a_v + col * NP + p, PA * NP);
  }
  __syncthreads();

  // ---------------- stage B: U, the 36-tap gather and the mask, per strip of SW same-parity grid columns
  for (int item = threadIdx.x; item < KY * 2 * NS * NP; item += NT) {
    const int p = item % NP;
    int r = item / NP;
    const int s = r % NS;
    r /= NS;
    const int par = r & 1;   // parity of the strip's grid columns kx = par + 2 * (SW * s + j)
    const int k = r >> 1;
    const int ob = ((R + par) >> 1) + SW * s;  // gout column of strip position j, tap pair m: ob + j - m
    const int oyb = (R + k) >> 1;
    const float* gdr = s_gd + ((R + k) & 1) * TD + ((R + par) & 1);
    f2v gv[SW];
#pragma unroll
    for (int j = 0; j < SW; ++j) gv[j] = f2v{0.f, 0.f};
#pragma unroll
    for (int my = 0; my < TD / DN; ++my) {
      f2v win[SW + TD / DN - 1];
#pragma unroll
      for (int i = 0; i < SW + TD / DN - 1; ++i) {
        const int col = ob - (TD / DN - 1) + i;
        win[i] = col < NOX ? g_s[((oyb - my) * PG + col) * NP + p] : f2v{0.f, 0.f};
      }
#pragma unroll
      for (int mx = 0; mx < TD / DN; ++mx) {
        const float w = gdr[(2 * my) * TD + 2 * mx];
#pragma unroll
        for (int j = 0; j < SW; ++j) gv[j] += w * win[j + (TD / DN - 1) - mx];
      }
    }
#pragma unroll
    for (int j = 0; j < SW; ++j) {
      const int kx = par + 2 * (SW * s + j);
      if (kx >= KX) break;
      const int jb = kx / UP;
      const int tb = UP - 1 - (kx - jb * UP);
      f2v u = f2v{0.f, 0.f};
#pragma unroll
      for (int m = 0; m < TU / UP; ++m) u += s_gu[tb + m * UP] * a_v[(k * PA + jb + m) * NP + p];
      f2v g = gv[j];
      g.x *= dact(u.x, a.slope, a.gain, a.lim);
      g.y *= dact(u.y, a.slope, a.gain, a.lim);
      b_v[(k * PB + kx) * NP + p] = g;
    }
  }
  __syncthreads();

  // ---------------- stage B2: horizontal down-by-up pass per grid row, over the row's a_v
  for (int item = threadIdx.x; item < KY * NP; item += NT) {
    const int k = item / NP;
    const int p = item - k * NP;
    f2v ch[TIX];
#pragma unroll
    for (int i = 0; i < TIX; ++i) ch[i] = f2v{0.f, 0.f};
#pragma unroll
    for (int kx = 0; kx < KX; ++kx) up_adjoint<UP, TU, TIX>(a.gu, kx, b_v[(k * PB + kx) * NP + p], ch);
#pragma unroll
    for (int i = 0; i < TIX; ++i) a_v[(k * PA + i) * NP + p] = ch[i];
  }
  __syncthreads();

  // ---------------- stage C: vertical down-by-up pass per column, store, ydot (flrelu_valu.h)
  TO* const gxn = reinterpret_cast<TO*>(a.gx) + (int64_t)n * a.in_h * a.in_w * a.c_p;
  bwd_stage_c<TI, UP, TU, KY, TIY, TIX, PA, NP, NT>(a, xin, a_v, blk, c0,
                                                    [=](int64_t e, f2v v) { store_pair_grad<TO>(gxn + e, v); });
}

// the gx tile and channel pairs per workgroup: what keeps the three f32 LDS arrays at or under 64 KiB
template <int UP> struct RbTile;
template <> struct RbTile<2> { static constexpr int TIY = 16, TIX = 16, NP = 2; };
template <> struct RbTile<4> { static constexpr int TIY = 8, TIX = 16, NP = 1; };
constexpr int RB_NT = 256;

template <int UP, int R>
static void rb_launch(const FlrRadBwdArgs& a, int ti, int tg, int grid, hipStream_t s) {
  using T = RbTile<UP>;
#define IC2_RB(TI_, TG_, TO_)                                                                                \
  hipLaunchKernelGGL((flrelu_radial_bwd_kernel<TI_, TG_, TO_, UP, 6 * UP, R, T::TIY, T::TIX, T::NP, RB_NT>), \
                     dim3(grid), dim3(RB_NT), 0, s, a)
  if (ti == IC2_F32) IC2_RB(float, float, float);
  else if (tg == IC2_F32) IC2_RB(_Float16, float, float);
  else if (tg == IC2_BF16) IC2_RB(_Float16, bf16_t, bf16_t);
  else IC2_RB(_Float16, _Float16, _Float16);
#undef IC2_RB
}

static void rb_tile(int up, int* tiy, int* tix, int* np) {
  if (up == 4) { *tiy = RbTile<4>::TIY; *tix = RbTile<4>::TIX; *np = RbTile<4>::NP; }
  else { *tiy = RbTile<2>::TIY; *tix = RbTile<2>::TIX; *np = RbTile<2>::NP; }
}

}  // namespace ic2

using namespace ic2;

extern "C" int64_t ic2_flrelu_bwd_2d_ydot_floats(int n, int c_p, int in_h, int in_w, int up) {
  if (n <= 0 || c_p <= 0 || in_h <= 0 || in_w <= 0) return 0;
  int tiy, tix, np;
  rb_tile(up, &tiy, &tix, &np);
  return (int64_t)n * ceil_div(in_h, tiy) * ceil_div(in_w, tix) * c_p;
}

extern "C" int ic2_flrelu_bwd_nhwc_2d(const void* x, int x_dtype, const void* gout, int g_dtype, void* gx, int gx_dtype,
                                      int n, int c_p, int in_h, int in_w, int out_h, int out_w, const float* fu,
                                      int fu_taps, const float* fd, int fd_taps, int up, int down, int px0, int px1,
                                      int py0, int py1, float gain, float slope, float clamp, int flip,
                                      const float* oscale, const float* bias, float* ydot, int64_t ydot_floats,
                                      void* stream) {
  const char* name = "flrelu_bwd_nhwc_2d";
  IC2_CHECK_ARG(x && gout && gx && fu && fd, "%s: null pointer", name);
  IC2_CHECK_ARG(n > 0 && c_p > 0 && in_h > 0 && in_w > 0 && up >= 1 && down >= 1, "%s: bad geometry", name);
  IC2_CHECK_ARG(fu_taps >= 1 && fd_taps >= 1, "%s: bad tap counts %d / %d", name, fu_taps, fd_taps);
  const bool cfg2 = up == 2 && down == 2 && fu_taps == 12 && fd_taps == RB_TD;
  const bool cfg4 = up == 4 && down == 2 && fu_taps == 24 && fd_taps == RB_TD;
  if (!cfg2 && !cfg4) {
    set_error("%s: no instance for up=%d down=%d taps=%d / %dx%d (up 2/4 with 6*up taps, down 2 with 12x12)", name, up,
              down, fu_taps, fd_taps, fd_taps);
    return IC2_E_UNSUPPORTED;
  }
  const int64_t ew = flr_out_size(in_w, up, px0, px1, fu_taps, fd_taps, down);
  const int64_t eh = flr_out_size(in_h, up, py0, py1, fu_taps, fd_taps, down);
  IC2_CHECK_ARG(out_h == eh && out_w == ew && out_h > 0 && out_w > 0, "%s: output %dx%d, expected %lldx%lld", name,
                out_h, out_w, (long long)eh, (long long)ew);
  if (px0 != py0) {
    set_error("%s: needs px0 == py0", name);
    return IC2_E_UNSUPPORTED;
  }
  if (!flr_act_ok(slope, gain)) {
    set_error("%s: needs 0 <= slope <= 1 and gain > 0", name);
    return IC2_E_UNSUPPORTED;
  }
  if (c_p % 16 != 0) {
    set_error("%s: c_p %d is not a multiple of 16", name, c_p);
    return IC2_E_UNSUPPORTED;
  }
  const bool t32 = x_dtype == IC2_F32 && g_dtype == IC2_F32 && gx_dtype == IC2_F32;
  const bool tbf = x_dtype == IC2_F16 && g_dtype == IC2_BF16 && gx_dtype == IC2_BF16;
  const bool t16 = x_dtype == IC2_F16 && g_dtype == IC2_F16 && gx_dtype == IC2_F16;
  const bool tmx = x_dtype == IC2_F16 && g_dtype == IC2_F32 && gx_dtype == IC2_F32;
  if (!t32 && !tbf && !t16 && !tmx) {
    set_error("%s: no instance for dtypes x=%d gout=%d gx=%d (f32/f32/f32, f16/bf16/bf16, f16/f16/f16, f16/f32/f32)",
              name, x_dtype, g_dtype, gx_dtype);
    return IC2_E_UNSUPPORTED;
  }
  int tiy, tix, np;
  rb_tile(up, &tiy, &tix, &np);
  const int64_t need = ic2_flrelu_bwd_2d_ydot_floats(n, c_p, in_h, in_w, up);
  IC2_CHECK_ARG(ydot == nullptr || ydot_floats >= need, "%s: ydot needs %lld floats", name, (long long)need);
  IC2_CHECK_ARG((int64_t)n * in_h * in_w * c_p < (1LL << 40) && (int64_t)in_h * up < (1 << 28) &&
                    (int64_t)in_w * up < (1 << 28) && std::abs(px0) < (1 << 20),
                "%s: geometry too large", name);
  FlrRadBwdArgs a;
  a.x = x; a.gout = gout; a.gx = gx;
  a.oscale = oscale; a.bias = bias; a.ydot = ydot;
  a.c_p = c_p; a.in_h = in_h; a.in_w = in_w; a.out_h = out_h; a.out_w = out_w; a.p0 = px0;
  a.slope = slope; a.gain = gain; a.lim = flr_lim(clamp, gain);
  a.tiles_x = (int)ceil_div(in_w, tix);
  a.tiles_y = (int)ceil_div(in_h, tiy);
  a.cblocks = c_p / (2 * np);
  const int64_t grid = (int64_t)n * a.tiles_y * a.tiles_x * a.cblocks;
  IC2_CHECK_ARG(grid < (1LL << 31), "%s: grid too large", name);
  flr_up_taps(a.gu, fu, fu_taps, up, flip);
  for (int ty = 0; ty < RB_TD; ++ty)
    for (int tx = 0; tx < RB_TD; ++tx)
      a.gd[ty * RB_TD + tx] = flip ? fd[ty * RB_TD + tx] : fd[(RB_TD - 1 - ty) * RB_TD + (RB_TD - 1 - tx)];
  hipStream_t s = as_stream(stream);
  const int R = flr_gout_phase(px0, fu_taps, fd_taps, down);
  if (cfg2) {
    if (R == 11) rb_launch<2, 11>(a, x_dtype, g_dtype, (int)grid, s);
    else rb_launch<2, 10>(a, x_dtype, g_dtype, (int)grid, s);
  } else {
    if (R == 11) rb_launch<4, 11>(a, x_dtype, g_dtype, (int)grid, s);
    else rb_launch<4, 10>(a, x_dtype, g_dtype, (int)grid, s);
  }
  IC2_CHECK_LAUNCH("flrelu_bwd_nhwc_2d");
  return IC2_OK;
}
