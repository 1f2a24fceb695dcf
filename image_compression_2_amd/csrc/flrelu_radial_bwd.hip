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
#include "common.h"

#include <cmath>

namespace ic2 {

typedef float rb2v __attribute__((ext_vector_type(2)));
typedef _Float16 rbh2 __attribute__((ext_vector_type(2)));

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

template <typename T> __device__ __forceinline__ rb2v rb_ld(const T* p, bool ok);
template <> __device__ __forceinline__ rb2v rb_ld<float>(const float* p, bool ok) {
  const float2 v = *reinterpret_cast<const float2*>(ok ? (const void*)p : zero_line());
  return rb2v{v.x, v.y};
}
template <> __device__ __forceinline__ rb2v rb_ld<_Float16>(const _Float16* p, bool ok) {
  const uint32_t u = *reinterpret_cast<const uint32_t*>(ok ? (const void*)p : zero_line());
  const rbh2 h = __builtin_bit_cast(rbh2, u);
  return rb2v{(float)h.x, (float)h.y};
}
template <> __device__ __forceinline__ rb2v rb_ld<bf16_t>(const bf16_t* p, bool ok) {
  const uint32_t u = *reinterpret_cast<const uint32_t*>(ok ? (const void*)p : zero_line());
  return rb2v{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
}

// gradient stores: f16 converts IEEE (overflow -> inf for the loss scaler), never saturated
template <typename T> __device__ __forceinline__ void rb_st(T* p, rb2v v);
template <> __device__ __forceinline__ void rb_st<float>(float* p, rb2v v) {
  *reinterpret_cast<float2*>(p) = make_float2(v.x, v.y);
}
template <> __device__ __forceinline__ void rb_st<bf16_t>(bf16_t* p, rb2v v) {
  *reinterpret_cast<uint32_t*>(p) = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
}
template <> __device__ __forceinline__ void rb_st<_Float16>(_Float16* p, rb2v v) {
  const rbh2 h = rbh2{(_Float16)v.x, (_Float16)v.y};
  *reinterpret_cast<uint32_t*>(p) = __builtin_bit_cast(uint32_t, h);
}

__device__ __forceinline__ float rb_dact(float u, float slope, float gain, float lim) {
  const float l = u > 0.f ? u : u * slope;
  return fabsf(l) < lim ? (u > 0.f ? gain : gain * slope) : 0.f;
}

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
  __shared__ __attribute__((aligned(16))) rb2v a_v[KY * PA * NP];
  __shared__ __attribute__((aligned(16))) rb2v b_v[KY * PB * NP];
  __shared__ __attribute__((aligned(16))) rb2v g_s[NOY * PG * NP];
  __shared__ float s_gd[TD * TD];
  __shared__ float s_gu[TU];
  static_assert(sizeof(rb2v) * (KY * PA + KY * PB + NOY * PG) * NP + 4 * (TD * TD + TU) <= 64 * 1024,
                "two workgroups per CU");

  int bid = blockIdx.x;
  const int cb = bid % a.cblocks;
  bid /= a.cblocks;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const int n = bid / a.tiles_y;
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
    const rb2v v = rb_ld<TG>(gin + ((int64_t)oy * a.out_w + ox) * a.c_p + c0 + 2 * p, ok);
    g_s[(orow * PG + oc) * NP + p] = ok ? v : rb2v{0.f, 0.f};
  }
  for (int item = threadIdx.x; item < NJX * NP; item += NT) {
    const int col = item / NP;
    const int p = item - col * NP;
    const int ix = j0x + col;
    const bool cok = (unsigned)ix < (unsigned)a.in_w;
    const TI* pc = xin + (int64_t)ix * a.c_p + c0 + 2 * p;
    rb2v in[NJY];
#pragma unroll
    for (int j = 0; j < NJY; ++j) {
      const int iy = j0y + j;
      const bool ok = cok && (unsigned)iy < (unsigned)a.in_h;
      const rb2v v = rb_ld<TI>(pc + (int64_t)iy * a.in_w * a.c_p, ok);
      in[j] = ok ? v : rb2v{0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < KY; ++k) {
      rb2v acc = rb2v{0.f, 0.f};
#pragma unroll
      for (int m = 0; m < TU / UP; ++m) {
        const int j = k / UP + m;
        const int t = (j + 1) * UP - 1 - k;
        if (j < NJY && t >= 0 && t < TU) acc += a.gu[t] * in[j];
      }
      a_v[(k * PA + col) * NP + p] = acc;
    }
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
    rb2v gv[SW];
#pragma unroll
    for (int j = 0; j < SW; ++j) gv[j] = rb2v{0.f, 0.f};
#pragma unroll
    for (int my = 0; my < TD / DN; ++my) {
      rb2v win[SW + TD / DN - 1];
#pragma unroll
      for (int i = 0; i < SW + TD / DN - 1; ++i) {
        const int col = ob - (TD / DN - 1) + i;
        win[i] = col < NOX ? g_s[((oyb - my) * PG + col) * NP + p] : rb2v{0.f, 0.f};
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
      rb2v u = rb2v{0.f, 0.f};
#pragma unroll
      for (int m = 0; m < TU / UP; ++m) u += s_gu[tb + m * UP] * a_v[(k * PA + jb + m) * NP + p];
      rb2v g = gv[j];
      g.x *= rb_dact(u.x, a.slope, a.gain, a.lim);
      g.y *= rb_dact(u.y, a.slope, a.gain, a.lim);
      b_v[(k * PB + kx) * NP + p] = g;
    }
  }
  __syncthreads();

  // ---------------- stage B2: horizontal down-by-up pass per grid row, over the row's a_v
  for (int item = threadIdx.x; item < KY * NP; item += NT) {
    const int k = item / NP;
    const int p = item - k * NP;
    rb2v ch[TIX];
#pragma unroll
    for (int i = 0; i < TIX; ++i) ch[i] = rb2v{0.f, 0.f};
#pragma unroll
    for (int kx = 0; kx < KX; ++kx) {
      const rb2v g = b_v[(k * PB + kx) * NP + p];
#pragma unroll
      for (int m = 0; m < TU / UP; ++m) {  // outputs i with 0 <= i*UP + TU - 1 - kx < TU
        const int i = (kx - TU + UP + UP * TU) / UP - TU + m;  // ceil((kx - TU + 1) / UP) + m, kept >= 0 inside
        const int t = i * UP + TU - 1 - kx;
        if (i >= 0 && i < TIX && t >= 0 && t < TU) ch[i] += a.gu[t] * g;
      }
    }
#pragma unroll
    for (int i = 0; i < TIX; ++i) a_v[(k * PA + i) * NP + p] = ch[i];
  }
  __syncthreads();

  // ---------------- stage C: vertical down-by-up pass per column, store (flrelu_bwd.hip's stage C)
  constexpr int S3 = (TIY % 2 == 0 && TIX * NP * 2 <= NT) ? 2 : 1;
  constexpr int RG = TIY / S3;
  constexpr int RGK = (RG - 1) * UP + TU;
  constexpr int NITEM = TIX * NP * S3;
  static_assert(NITEM <= NT && NITEM <= KY * PA * NP, "stage C: one item per thread, ydot partials in a_v");
  rb2v ydp = rb2v{0.f, 0.f};
  const int item = threadIdx.x;
  const int p = item % NP;
  const int c = c0 + 2 * p;
  if (item < NITEM) {
    const int ix = (item / NP) % TIX;
    const int rg = item / (NP * TIX);
    const int gxx = i0x + ix;
    if (gxx < a.in_w) {
      rb2v o[RG];
#pragma unroll
      for (int r = 0; r < RG; ++r) o[r] = rb2v{0.f, 0.f};
      const int kb = rg * RG * UP;
#pragma unroll
      for (int kk = 0; kk < RGK; ++kk) {
        const rb2v v = a_v[((kb + kk) * PA + ix) * NP + p];
#pragma unroll
        for (int m = 0; m < TU / UP; ++m) {
          const int r = (kk - TU + UP + UP * TU) / UP - TU + m;
          const int t = r * UP + TU - 1 - kk;
          if (r >= 0 && r < RG && t >= 0 && t < TU) o[r] += a.gu[t] * v;
        }
      }
      rb2v os = rb2v{1.f, 1.f}, bi = rb2v{0.f, 0.f};
      if (a.oscale) os = rb2v{a.oscale[(int64_t)n * a.c_p + c], a.oscale[(int64_t)n * a.c_p + c + 1]};
      if (a.bias) bi = rb2v{a.bias[c], a.bias[c + 1]};
      if (a.ydot) {  // the ydot operand x of every row before the first gx store (flrelu_bwd.hip)
        rb2v xv[RG];
#pragma unroll
        for (int r = 0; r < RG; ++r) {
          const int gyy = i0y + rg * RG + r;
          xv[r] = rb_ld<TI>(xin + ((int64_t)gyy * a.in_w + gxx) * a.c_p + c, gyy < a.in_h);
        }
#pragma unroll
        for (int r = 0; r < RG; ++r)
          if (i0y + rg * RG + r < a.in_h) ydp += o[r] * (xv[r] - bi);
      }
#pragma unroll
      for (int r = 0; r < RG; ++r) {
        const int gyy = i0y + rg * RG + r;
        if (gyy >= a.in_h) continue;
        const int64_t e = ((int64_t)gyy * a.in_w + gxx) * a.c_p + c;
        rb_st<TO>(reinterpret_cast<TO*>(a.gx) + (int64_t)n * a.in_h * a.in_w * a.c_p + e, o[r] * os);
      }
    }
  }
  if (a.ydot) {  // fixed-order reduction of the tile's items per channel pair (LDS reused after a barrier)
    __syncthreads();
    if (item < NITEM) a_v[item] = ydp;
    __syncthreads();
    if (item < NP) {
      rb2v t = rb2v{0.f, 0.f};
      for (int k = item; k < NITEM; k += NP) t += a_v[k];
      const int tile = ty * a.tiles_x + tx;
      float* py = a.ydot + ((int64_t)n * a.tiles_y * a.tiles_x + tile) * a.c_p + c;
      py[0] = t.x;
      py[1] = t.y;
    }
  }
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
  const int64_t ew = ((int64_t)in_w * up + (px0 + px1) - (fu_taps - 1) - (fd_taps - 1) + (down - 1)) / down;
  const int64_t eh = ((int64_t)in_h * up + (py0 + py1) - (fu_taps - 1) - (fd_taps - 1) + (down - 1)) / down;
  IC2_CHECK_ARG(out_h == eh && out_w == ew && out_h > 0 && out_w > 0, "%s: output %dx%d, expected %lldx%lld", name,
                out_h, out_w, (long long)eh, (long long)ew);
  if (px0 != py0) {
    set_error("%s: needs px0 == py0", name);
    return IC2_E_UNSUPPORTED;
  }
  if (!(slope >= 0.f && slope <= 1.f && gain > 0.f)) {
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
  a.slope = slope; a.gain = gain; a.lim = clamp >= 0.f ? clamp / gain : INFINITY;
  a.tiles_x = (int)ceil_div(in_w, tix);
  a.tiles_y = (int)ceil_div(in_h, tiy);
  a.cblocks = c_p / (2 * np);
  const int64_t grid = (int64_t)n * a.tiles_y * a.tiles_x * a.cblocks;
  IC2_CHECK_ARG(grid < (1LL << 31), "%s: grid too large", name);
  for (int t = 0; t < 24; ++t) a.gu[t] = 0.f;
  for (int t = 0; t < fu_taps; ++t) a.gu[t] = (flip ? fu[t] : fu[fu_taps - 1 - t]) * (float)up;
  for (int ty = 0; ty < RB_TD; ++ty)
    for (int tx = 0; tx < RB_TD; ++tx)
      a.gd[ty * RB_TD + tx] = flip ? fd[ty * RB_TD + tx] : fd[(RB_TD - 1 - ty) * RB_TD + (RB_TD - 1 - tx)];
  hipStream_t s = as_stream(stream);
  // gout phase: R = td - 1 - ph with ph = (-(p0 - tu + 1 - td + 1)) mod down (up % down == 0: same for every tile)
  const int q = px0 - fu_taps + 1 - fd_taps + 1;
  const int ph = ((-q) % down + down) % down;
  const int R = fd_taps - 1 - ph;
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
