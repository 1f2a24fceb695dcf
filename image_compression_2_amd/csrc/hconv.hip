// Halo direct conv for narrow 3x3 layers (cin_p <= 96, cout_p <= 64; bf16): the encoder's block 0 and from_rgb
// and the SG3-T-1024 tail (L11_1044_51, L12_1044_32, L13_1024_32) at >= 256^2.  There the implicit GEMM (igemm.hip) re-fetches
// every input pixel once per tap (9 shifted 256-pixel panels per 32 channels) for only 32-64 MACs per
// fetched element, and its per-chunk barrier guards 8-16 MFMAs.  Here a persistent workgroup keeps the
// whole packed weight [cout_p][9][cin_p] in LDS, stages one (TH+2) x (32+2) x cin_p input halo per
// TH x 32-pixel output tile (TH = 8, or 4 at 96 channels; fetched once: 1.6x instead of 9x), and runs all 9 * cin_p/32 K-steps without
// a barrier.  The next tile's halo is loaded into registers while the current tile computes.
// Wave w of 8 owns pixel blocks {w, w+8, ...} (16 pixels of one row) x every 16-channel o-block:
// A = weights (lane: o = 16i + fr, k = 8 fh .. +7), B = halo pixels (lane: pixel fr, k = 8 fh .. +7).
// Epilogue = ig_store4 (same oscale / bias / activation / output layouts as the implicit GEMM).
// (This file also holds the 1x1 ToRGB kernel, below: it shares nothing with the GEMMs either.)
#include "conv_plan.h"

namespace ic2 {

template <int CINP, int COUTP, int TH>
struct HcCfg {
  static constexpr int TW = 32, HR = TH + 2, HC = TW + 2;
  static constexpr int PPB = CINP * 2 + 16;          // halo pixel pitch (bytes): 16 lanes hit distinct banks
  static constexpr int WPB = 9 * CINP * 2 + 16;      // weight row pitch (bytes)
  static constexpr int HALO_B = HR * HC * PPB, W_B = COUTP * WPB;
  static constexpr int CB = CINP / 32, OB = COUTP / 16, JB = TH * 2 / 8;
  static constexpr int NPIECE = HR * HC * (CINP / 8);  // 16-B pieces per halo
  static constexpr int PER_T = (NPIECE + 511) / 512;
};

template <int CINP, int COUTP, int TH, bool F16 = false>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(CINP == 32 ? 4 : 1)))
hconv_kernel(IgemmArgs a, int tiles_x, int tiles_y, int ntiles) {
  using C = HcCfg<CINP, COUTP, TH>;
  __shared__ __attribute__((aligned(16))) char lds[C::HALO_B + C::W_B];
  char* const halo = lds;
  char* const wts = lds + C::HALO_B;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fh = lane >> 4;

  // packed weight -> LDS, once per workgroup
  const char* wg = reinterpret_cast<const char*>(a.w);
  constexpr int WPIECE = 9 * CINP / 8;
  for (int e = tid; e < COUTP * WPIECE; e += 512) {
    const int o = e / WPIECE, r = e - o * WPIECE;
    *reinterpret_cast<uint4*>(wts + o * C::WPB + r * 16) =
        *reinterpret_cast<const uint4*>(wg + ((int64_t)o * 9 * CINP + r * 8) * 2);
  }

  const char* xg = reinterpret_cast<const char*>(a.x);
  uint4 pre[C::PER_T];
  auto fetch = [&](int t) {
    const int tx = t % tiles_x;
    const int t2 = t / tiles_x;
    const int ty = t2 % tiles_y;
    const int nn = t2 / tiles_y;
    const int y0 = ty * TH - a.pad, x0 = tx * C::TW - a.pad;
#pragma unroll
    for (int k = 0; k < C::PER_T; ++k) {
      const int e = tid + 512 * k;
      const int pi = e / (CINP / 8), part = e - pi * (CINP / 8);
      const int hr = pi / C::HC, hc = pi - hr * C::HC;
      const int iy = y0 + hr, ix = x0 + hc;
      const bool ok = e < C::NPIECE && (unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w_;
      pre[k] = ok ? *reinterpret_cast<const uint4*>(xg + ((((int64_t)nn * a.h + iy) * a.w_ + ix) * CINP + part * 8) * 2)
                  : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  if (blockIdx.x < ntiles) fetch(blockIdx.x);

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    __syncthreads();  // the previous tile's halo reads (and the weight stores) are done
#pragma unroll
    for (int k = 0; k < C::PER_T; ++k) {
      const int e = tid + 512 * k;
      if (e < C::NPIECE) {
        const int pi = e / (CINP / 8), part = e - pi * (CINP / 8);
        *reinterpret_cast<uint4*>(halo + pi * C::PPB + part * 16) = pre[k];
      }
    }
    __syncthreads();
    if (t + (int)gridDim.x < ntiles) fetch(t + gridDim.x);  // in flight during this tile's MFMAs

    f32x4 acc[C::OB][C::JB];
#pragma unroll
    for (int i = 0; i < C::OB; ++i)
#pragma unroll
      for (int j = 0; j < C::JB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * (tap / 3);
#pragma unroll
      for (int cb = 0; cb < C::CB; ++cb) {
        bf16x8 bfr[C::JB], af[C::OB];
#pragma unroll
        for (int j = 0; j < C::JB; ++j) {
          const int pb = wave + 8 * j;
          const int r = pb >> 1, c0 = (pb & 1) * 16;
          bfr[j] = *reinterpret_cast<const bf16x8*>(halo + ((r + ky) * C::HC + c0 + kx + fr) * C::PPB + cb * 64 +
                                                    fh * 16);
        }
#pragma unroll
        for (int i = 0; i < C::OB; ++i)
          af[i] = *reinterpret_cast<const bf16x8*>(wts + (16 * i + fr) * C::WPB + (tap * CINP + cb * 32) * 2 + fh * 16);
#pragma unroll
        for (int i = 0; i < C::OB; ++i)
#pragma unroll
          for (int j = 0; j < C::JB; ++j)
            acc[i][j] = mfma32<F16>(af[i], bfr[j], acc[i][j]);
      }
    }

    const int tx = t % tiles_x;
    const int t2 = t / tiles_x;
    const int ty = t2 % tiles_y;
    const int nn = t2 / tiles_y;
    // every channel block's operands before the first store (see ig_load_oscale); not in the 32 -> 64 instance,
    // whose 4-waves-per-SIMD register budget (128) would spill them (measured 142 -> 179 us on e0a) and whose
    // occupancy hides the per-block loads instead
    constexpr bool kPre = !(CINP == 32 && COUTP == 64);
    float4 sc[C::OB], bi[C::OB];
    if constexpr (kPre) {
#pragma unroll
      for (int i = 0; i < C::OB; ++i) {
        sc[i] = ig_load_oscale(a, nn, 16 * i + 4 * fh);
        bi[i] = ig_load_bias(a, 16 * i + 4 * fh);
      }
      ig_preloads_done();
    }
#pragma unroll
    for (int j = 0; j < C::JB; ++j) {
      const int pb = wave + 8 * j;
      const int oy = ty * TH + (pb >> 1), ox = tx * C::TW + (pb & 1) * 16 + fr;
      if (oy >= a.ho || ox >= a.wo) continue;
      const int pix = oy * a.wo + ox;
      const int p = nn * a.ho * a.wo + pix;
#pragma unroll
      for (int i = 0; i < C::OB; ++i) {
        const float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
        if constexpr (!kPre) {
          sc[i] = ig_load_oscale(a, nn, 16 * i + 4 * fh);
          bi[i] = ig_load_bias(a, 16 * i + 4 * fh);
        }
        ig_store4v(a, p, nn, pix, 16 * i + 4 * fh, v, sc[i], bi[i]);
      }
    }
  }
}

template <int CINP, int COUTP, bool F16>
static void launch_hconv_t(const IgemmArgs& a, hipStream_t s) {
  constexpr int TH = CINP > 64 ? 4 : 8;  // 96 channels: 4-row tiles keep halo + weight within 160 KB of LDS
  const int tiles_x = (int)ceil_div(a.wo, 32), tiles_y = (int)ceil_div(a.ho, TH);
  const int ntiles = a.n * tiles_x * tiles_y;
  static int resident = 0;
  if (resident == 0) {
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, hconv_kernel<CINP, COUTP, TH, F16>, 512, 0);
    resident = (cus > 0 ? cus : 256) * (per_cu > 0 ? per_cu : 1);
  }
  const int grid = ntiles < resident ? ntiles : resident;
  hipLaunchKernelGGL((hconv_kernel<CINP, COUTP, TH, F16>), dim3((unsigned)grid), dim3(512), 0, s, a, tiles_x,
                     tiles_y, ntiles);
}
// the instance of a's cin_p in {32, 64, 96} x cout_p in {32, 64} (hconv_eligible, conv_dispatch.hip)
template <bool F16>
static void launch_hconv_cfg(const IgemmArgs& a, hipStream_t s) {
  if (a.cin_p == 32 && a.cout_p == 32) launch_hconv_t<32, 32, F16>(a, s);
  else if (a.cin_p == 32) launch_hconv_t<32, 64, F16>(a, s);
  else if (a.cin_p == 64 && a.cout_p == 32) launch_hconv_t<64, 32, F16>(a, s);
  else if (a.cin_p == 64) launch_hconv_t<64, 64, F16>(a, s);
  else if (a.cout_p == 32) launch_hconv_t<96, 32, F16>(a, s);
  else launch_hconv_t<96, 64, F16>(a, s);
}
void launch_hconv(const IgemmArgs& a, bool f16, hipStream_t s) {
  if (f16) launch_hconv_cfg<true>(a, s);
  else launch_hconv_cfg<false>(a, s);
}

// ------------------------------------------------------------------------------------------------
// ToRGB (1x1 conv to <= 4 channels, NCHW f32 output; SG3 SynthesisLayer L14, is_torgb): HBM-bound, so a
// VALU dot product instead of a 32-row MFMA tile that is 29/32 padding.  L = cin_p/16 lanes per pixel,
// 16 channels (2 x 16 B) each, a fixed xor-shuffle tree over the L lanes, then the igemm epilogue math
// (oscale, bias, activation / clamp, out_mul) on the group's first lane.
// 2-byte element -> f32 (bf16: the high half; f16: a conversion)
template <bool F16>
__device__ __forceinline__ float h2f(uint32_t bits16) {
  if constexpr (F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
  else return __uint_as_float(bits16 << 16);
}

template <int L, int CV, bool F16 = false>
__global__ void __launch_bounds__(256) torgb_kernel(IgemmArgs a) {
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int sub = threadIdx.x & (L - 1);
  const int hw = a.ho * a.wo;
  float wv[CV][16];
  const uint16_t* wg = reinterpret_cast<const uint16_t*>(a.w);
#pragma unroll
  for (int o = 0; o < CV; ++o)
#pragma unroll
    for (int k = 0; k < 16; ++k) wv[o][k] = h2f<F16>(wg[(int64_t)o * a.cin_p + sub * 16 + k]);
  float bi[CV];
#pragma unroll
  for (int o = 0; o < CV; ++o) bi[o] = a.bias ? a.bias[o] : 0.f;
  const uint16_t* xg = reinterpret_cast<const uint16_t*>(a.x);
  float* yo = reinterpret_cast<float*>(a.y);
  const int stride = gridDim.x * (256 / L);
  for (int p = tid / L; p < a.M; p += stride) {
    // the lane's 16 channels of pixel p: 32 B of the pixel (NHWC) or of plane `sub` of the pixel's sample (blocked)
    const uint4* src = reinterpret_cast<const uint4*>(
        a.x_pix == 16 ? xg + (int64_t)(p / hw) * a.x_img + ((int64_t)sub * hw + p % hw) * 16
                               : xg + (int64_t)p * a.cin_p + sub * 16);
    const uint4 u0 = src[0], u1 = src[1];
    const uint32_t w32[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
    float acc[CV];
#pragma unroll
    for (int o = 0; o < CV; ++o) acc[o] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float lo = h2f<F16>(w32[k] & 0xffffu), hi = h2f<F16>(w32[k] >> 16);
#pragma unroll
      for (int o = 0; o < CV; ++o) acc[o] = fmaf(wv[o][2 * k + 1], hi, fmaf(wv[o][2 * k], lo, acc[o]));
    }
#pragma unroll
    for (int m = 1; m < L; m <<= 1)
#pragma unroll
      for (int o = 0; o < CV; ++o) acc[o] += __shfl_xor(acc[o], m, 64);
    if (sub == 0) {
      const int nn = p / hw, pix = p - nn * hw;
#pragma unroll
      for (int o = 0; o < CV; ++o) {
        if (o >= a.cout_valid) break;
        float t = acc[o] * (a.oscale ? a.oscale[(int64_t)nn * a.cout_p + o] : 1.f) + bi[o];
        if (a.act) t = lrelu_gain_clamp(t, a.slope, a.act_gain, a.clamp);
        yo[((int64_t)nn * a.cout_valid + o) * hw + pix] = t * a.out_mul;
      }
    }
  }
}

template <bool F16>
static void launch_torgb_t(const IgemmArgs& a, hipStream_t s) {
  const int L = a.cin_p / 16;
  const int64_t need = ceil_div((int64_t)a.M * L, 256);
  const unsigned grid = (unsigned)(need < 8192 ? need : 8192);
  if (L == 2) hipLaunchKernelGGL((torgb_kernel<2, 4, F16>), dim3(grid), dim3(256), 0, s, a);
  else if (L == 4) hipLaunchKernelGGL((torgb_kernel<4, 4, F16>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((torgb_kernel<8, 4, F16>), dim3(grid), dim3(256), 0, s, a);
}
void launch_torgb(const IgemmArgs& a, bool f16, hipStream_t s) {
  if (f16) launch_torgb_t<true>(a, s);
  else launch_torgb_t<false>(a, s);
}

}  // namespace ic2
