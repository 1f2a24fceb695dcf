// What the four VALU filtered-lrelu kernels share (flrelu.hip / flrelu_radial.hip: forward with a separable / a 2-D
// down filter; flrelu_bwd.hip / flrelu_radial_bwd.hip: their backwards): channel-pair access, the activation, the
// polyphase up-FIR and its adjoint, the backward's stage-A up-FIR rows and stage C, and the host side's geometry,
// admissibility and tap preparation.  The MFMA kernels (flrelu_mfma.h) share none of this.
//
// These functions are compiled on their own before they are inlined into a kernel, and that changes the code: the
// column loads of the vertical passes (forward stage 1, backward stage A), shared, came out with SGPRs spilled to
// VGPR lanes and more VGPRs than inline, so they stay in the kernels (profiles/r20_flr_valu_share.txt).
#pragma once
#include "common.h"

#include <cmath>
#include <type_traits>

namespace ic2 {

// ------------------------------------------------------------------------------------------------
// channel pairs: lanes own two adjacent channels, f32 math
// ------------------------------------------------------------------------------------------------
typedef float f2v __attribute__((ext_vector_type(2)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t bf16_pack(f2v v) { return (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16); }
__device__ __forceinline__ f2v bf16_unpack(uint32_t v) {
  return f2v{__uint_as_float(v << 16), __uint_as_float(v & 0xffff0000u)};
}
__device__ __forceinline__ h2v f16_sat(f2v v) {
  return h2v{(_Float16)__builtin_amdgcn_fmed3f(v.x, -65504.f, 65504.f),
             (_Float16)__builtin_amdgcn_fmed3f(v.y, -65504.f, 65504.f)};
}

// Branch-free pair load: an out-of-range sample reads the code object's zero line and is then
// masked, so no load sits behind a branch (hipcc would otherwise wait vmcnt(0) per element).
template <typename T> __device__ __forceinline__ f2v load_pair(const T* p, bool ok);
template <> __device__ __forceinline__ f2v load_pair<float>(const float* p, bool ok) {
  const float2 v = *reinterpret_cast<const float2*>(ok ? (const void*)p : zero_line());
  return f2v{v.x, v.y};
}
template <> __device__ __forceinline__ f2v load_pair<bf16_t>(const bf16_t* p, bool ok) {
  return bf16_unpack(*reinterpret_cast<const uint32_t*>(ok ? (const void*)p : zero_line()));
}
template <> __device__ __forceinline__ f2v load_pair<_Float16>(const _Float16* p, bool ok) {
  const h2v v = *reinterpret_cast<const h2v*>(ok ? (const void*)p : zero_line());
  return f2v{(float)v.x, (float)v.y};
}

// Pair stores.  f16 has two policies on purpose: a forward output saturates (as Elem<_Float16>), a gradient
// converts IEEE (overflow -> inf, which the loss scaler must see).
__device__ __forceinline__ void store_pair(float* p, f2v v) { *reinterpret_cast<float2*>(p) = make_float2(v.x, v.y); }
__device__ __forceinline__ void store_pair(bf16_t* p, f2v v) { *reinterpret_cast<uint32_t*>(p) = bf16_pack(v); }
__device__ __forceinline__ void store_pair_f16_sat(_Float16* p, f2v v) { *reinterpret_cast<h2v*>(p) = f16_sat(v); }
__device__ __forceinline__ void store_pair_f16_ieee(_Float16* p, f2v v) {
  *reinterpret_cast<h2v*>(p) = h2v{(_Float16)v.x, (_Float16)v.y};
}
template <typename T> __device__ __forceinline__ void store_pair_fwd(T* p, f2v v) {
  if constexpr (std::is_same<T, _Float16>::value) store_pair_f16_sat(p, v);
  else store_pair(p, v);
}
template <typename T> __device__ __forceinline__ void store_pair_grad(T* p, f2v v) {
  if constexpr (std::is_same<T, _Float16>::value) store_pair_f16_ieee(p, v);
  else store_pair(p, v);
}

// LDS storage of a pair: f32 (parity paths), packed bf16 (flrelu.hip's bf16 path: halves the LDS footprint ->
// twice the resident workgroups; one extra rounding of the vertically up-sampled input, below the bf16 rounding of
// the output itself) or f16 (flrelu_radial.hip's 16-bit paths; saturating: the vertically up-sampled input may
// pass the f16 range by the filter's overshoot).
template <typename LT> struct LdsPair;
template <> struct LdsPair<f2v> {
  __device__ static __forceinline__ f2v pack(f2v v) { return v; }
  __device__ static __forceinline__ f2v unpack(f2v v) { return v; }
};
template <> struct LdsPair<uint32_t> {
  __device__ static __forceinline__ uint32_t pack(f2v v) { return bf16_pack(v); }
  __device__ static __forceinline__ f2v unpack(uint32_t v) { return bf16_unpack(v); }
};
template <> struct LdsPair<h2v> {
  __device__ static __forceinline__ h2v pack(f2v v) { return f16_sat(v); }
  __device__ static __forceinline__ f2v unpack(h2v v) { return f2v{(float)v.x, (float)v.y}; }
};

// lrelu + clamp on a channel pair in 5 instructions: one packed multiply, two max (slope <= 1 makes
// lrelu(v) = max(v, slope*v)) and two med3 clamps.  The gain is folded into the down taps
// and the clamp bound divided by it: clamp(gain*lrelu(v), +-c) = gain * clamp(lrelu(v), +-c/gain).
__device__ __forceinline__ f2v act2(f2v v, float slope, float lim) {
  const f2v sv = v * slope;
  f2v r;
  r.x = __builtin_amdgcn_fmed3f(fmaxf(v.x, sv.x), -lim, lim);
  r.y = __builtin_amdgcn_fmed3f(fmaxf(v.y, sv.y), -lim, lim);
  return r;
}
// its derivative w.r.t. the up-sampled value u, gain included
__device__ __forceinline__ float dact(float u, float slope, float gain, float lim) {
  const float l = u > 0.f ? u : u * slope;
  return fabsf(l) < lim ? (u > 0.f ? gain : gain * slope) : 0.f;
}

// blockIdx.x = ((n * tiles_y + ty) * tiles_x + tx) * cblocks + cb
struct FlrBlock {
  int cb, tx, ty, n;
};
template <typename A> __device__ __forceinline__ FlrBlock flr_block(const A& a) {
  FlrBlock b;
  int bid = blockIdx.x;
  b.cb = bid % a.cblocks;
  bid /= a.cblocks;
  b.tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  b.ty = bid % a.tiles_y;
  b.n = bid / a.tiles_y;
  return b;
}

// ------------------------------------------------------------------------------------------------
// forward: polyphase up-FIR
// ------------------------------------------------------------------------------------------------
// First input sample j whose up-FIR tap t = U*j + DELTA - i lies in [0, TU): j = ceil((i - DELTA) / U),
// clamped at 0.  The TU/U samples j, j+1, ... are exactly the polyphase taps of grid position i.
template <int U, int DELTA>
__host__ __device__ constexpr int up_first(int i) {
  return i < DELTA ? 0 : (i - DELTA + U - 1) / U;
}

// grid position i (a compile-time constant once the caller's loop is unrolled) from the N samples in[]
template <int U, int TU, int DELTA, int N>
__device__ __forceinline__ f2v up_fir(const float* gu, int i, const f2v* in) {
  f2v acc = f2v{0.f, 0.f};
#pragma unroll
  for (int m = 0; m < TU / U; ++m) {  // the TU/U polyphase taps landing on grid position i
    const int j = up_first<U, DELTA>(i) + m;
    if (j < N) acc += gu[U * j + DELTA - i] * in[j];
  }
  return acc;
}

// ------------------------------------------------------------------------------------------------
// backward: shared stages (A = the kernel's argument struct: FlrBwdArgs or FlrRadBwdArgs)
// ------------------------------------------------------------------------------------------------
// Stage A, the x half: the NJY samples in[] of one x column (rows from the tile's first, zero outside the image) ->
// vertical up-FIR -> the KY rows of U at dst[k * pitch].
template <int UP, int TU, int KY, int NJY>
__device__ __forceinline__ void bwd_up_rows(const float* gu, const f2v* in, f2v* dst, int pitch) {
#pragma unroll
  for (int k = 0; k < KY; ++k) {
    f2v acc = f2v{0.f, 0.f};
#pragma unroll
    for (int m = 0; m < TU / UP; ++m) {
      const int j = k / UP + m;
      const int t = (j + 1) * UP - 1 - k;
      if (j < NJY && t >= 0 && t < TU) acc += gu[t] * in[j];
    }
    dst[k * pitch] = acc;
  }
}

// Adjoint up-FIR scatter: grid sample g at tile-local grid index k adds gu[t] * g to the outputs i with
// 0 <= t = i*UP + TU - 1 - k < TU.  Both axes of both backward kernels.
template <int UP, int TU, int NOUT>
__device__ __forceinline__ void up_adjoint(const float* gu, int k, f2v g, f2v* out) {
#pragma unroll
  for (int m = 0; m < TU / UP; ++m) {
    const int i = (k - TU + UP + UP * TU) / UP - TU + m;  // ceil((k - TU + 1) / UP) + m, kept >= 0 inside
    const int t = i * UP + TU - 1 - k;
    if (i >= 0 && i < NOUT && t >= 0 && t < TU) out[i] += gu[t] * g;
  }
}

// Stage C: vertical down-by-up pass per column of a_v (KY rows of pitch PA), then the optional epilogue of the
// modulated conv's backward (x = conv * oscale + bias): gx * oscale is stored through store(e, v) (e = element index
// within the sample; dtype and f16 policy are the caller's), and sum gx * (x - bias) over the tile goes to ydot
// -> d oscale = sum / oscale on the host.
template <typename TI, int UP, int TU, int KY, int TIY, int TIX, int PA, int NP, int NT, typename A, typename ST>
__device__ __forceinline__ void bwd_stage_c(const A& a, const TI* xin, f2v* a_v, FlrBlock b, int c0, ST store) {
  constexpr int S3 = (TIY % 2 == 0 && TIX * NP * 2 <= NT) ? 2 : 1;
  constexpr int RG = TIY / S3;
  constexpr int RGK = (RG - 1) * UP + TU;
  constexpr int NITEM = TIX * NP * S3;
  static_assert(NITEM <= NT && NITEM <= KY * PA * NP, "stage C: one item per thread, ydot partials in a_v");
  // every field read after a store, by value: compiled stand-alone ahead of inlining, a store through gx or a_v may
  // alias the struct, and the field would be read again (and its index arithmetic redone) per row
  const int in_h = a.in_h, in_w = a.in_w, c_p = a.c_p, tiles_x = a.tiles_x, tiles_y = a.tiles_y;
  float* const ydot = a.ydot;
  const int n = b.n, i0y = b.ty * TIY, i0x = b.tx * TIX;
  f2v ydp = f2v{0.f, 0.f};
  const int item = threadIdx.x;
  const int p = item % NP;
  const int c = c0 + 2 * p;
  if (item < NITEM) {
    const int ix = (item / NP) % TIX;
    const int rg = item / (NP * TIX);
    const int gxx = i0x + ix;
    if (gxx < in_w) {
      f2v o[RG];
#pragma unroll
      for (int r = 0; r < RG; ++r) o[r] = f2v{0.f, 0.f};
      const int kb = rg * RG * UP;
#pragma unroll
      for (int kk = 0; kk < RGK; ++kk) up_adjoint<UP, TU, RG>(a.gu, kk, a_v[((kb + kk) * PA + ix) * NP + p], o);
      f2v os = f2v{1.f, 1.f}, bi = f2v{0.f, 0.f};
      if (a.oscale) os = f2v{a.oscale[(int64_t)n * c_p + c], a.oscale[(int64_t)n * c_p + c + 1]};
      if (a.bias) bi = f2v{a.bias[c], a.bias[c + 1]};
      // the ydot operand x of every row BEFORE the first gx store: a load placed after a store to gx may alias
      // it, which serialised one round trip per row (vmcnt(0) per row in the up-4 instances)
      if (ydot) {
        f2v xv[RG];
#pragma unroll
        for (int r = 0; r < RG; ++r) {
          const int gyy = i0y + rg * RG + r;
          xv[r] = load_pair<TI>(xin + ((int64_t)gyy * in_w + gxx) * c_p + c, gyy < in_h);
        }
#pragma unroll
        for (int r = 0; r < RG; ++r)
          if (i0y + rg * RG + r < in_h) ydp += o[r] * (xv[r] - bi);
      }
#pragma unroll
      for (int r = 0; r < RG; ++r) {
        const int gyy = i0y + rg * RG + r;
        if (gyy >= in_h) continue;
        store(((int64_t)gyy * in_w + gxx) * c_p + c, o[r] * os);
      }
    }
  }
  if (ydot) {  // fixed-order reduction of the tile's items per channel pair (LDS reused after a barrier)
    __syncthreads();
    if (item < NITEM) a_v[item] = ydp;
    __syncthreads();
    if (item < NP) {
      f2v t = f2v{0.f, 0.f};
      for (int k = item; k < NITEM; k += NP) t += a_v[k];
      const int tile = b.ty * tiles_x + b.tx;
      float* py = ydot + ((int64_t)n * tiles_y * tiles_x + tile) * c_p + c;
      py[0] = t.x;
      py[1] = t.y;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// output samples of one axis: zero-insert by up, pad / crop by p0 + p1, FIR fu_taps, FIR fd_taps, keep every down-th
inline int64_t flr_out_size(int in, int up, int p0, int p1, int fu_taps, int fd_taps, int down) {
  return ((int64_t)in * up + (p0 + p1) - (fu_taps - 1) - (fd_taps - 1) + (down - 1)) / down;
}
// the fused activation uses max(v, slope*v), and folds the gain into taps and clamp bound
inline bool flr_act_ok(float slope, float gain) { return slope >= 0.f && slope <= 1.f && gain > 0.f; }
// clamp bound on the gain-free activation (+inf: no clamp)
inline float flr_lim(float clamp, float gain) { return clamp >= 0.f ? clamp / gain : INFINITY; }
// NOTE: fu / fd are HOST pointers (filters are layer constants; they travel in the kernarg)
// up taps, flipped unless flip_filter, times up (the per-axis share of the up^2 gain); null = the 1-tap identity
inline void flr_up_taps(float (&gu)[24], const float* fu, int fu_taps, int up, int flip) {
  for (int t = 0; t < 24; ++t) gu[t] = 0.f;
  for (int t = 0; t < fu_taps; ++t) gu[t] = (fu ? (flip ? fu[t] : fu[fu_taps - 1 - t]) : 1.f) * (float)up;
}
// 1-D down taps, flipped unless flip_filter
inline void flr_down_taps(float (&gd)[12], const float* fd, int fd_taps, int flip) {
  for (int t = 0; t < 12; ++t) gd[t] = 0.f;
  for (int t = 0; t < fd_taps; ++t) gd[t] = fd ? (flip ? fd[t] : fd[fd_taps - 1 - t]) : 1.f;
}
// backward: gout phase R = td - 1 - ph with ph = (-(p0 - tu + 1 - td + 1)) mod down (up % down == 0: same for
// every tile)
inline int flr_gout_phase(int p0, int fu_taps, int fd_taps, int down) {
  const int q = p0 - fu_taps + 1 - fd_taps + 1;
  const int ph = ((-q) % down + down) % down;
  return fd_taps - 1 - ph;
}

}  // namespace ic2
