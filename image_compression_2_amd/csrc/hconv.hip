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

// lrelu((v - mean) * scale + shift) on 8 bf16 values, rounded back to bf16: the arithmetic of
// gn_apply_oct_kernel (encoder_ops.hip) on the same operands, so a fused input equals the materialised one bit for bit
__device__ __forceinline__ uint4 gn_lrelu_bf16x8(uint4 u, const float4 (&p)[8], float slope) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float lo = __uint_as_float(w[k] << 16), hi = __uint_as_float(w[k] & 0xffff0000u);
    lo = __builtin_fmaf(lo - p[2 * k].x, p[2 * k].y, p[2 * k].z);
    hi = __builtin_fmaf(hi - p[2 * k + 1].x, p[2 * k + 1].y, p[2 * k + 1].z);
    lo = lo < 0.f ? lo * slope : lo;
    hi = hi < 0.f ? hi * slope : hi;
    o[k] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

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

template <int CINP, int COUTP, int TH, bool GN, bool F16 = false>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(CINP == 32 ? 4 : 1)))
hconv_kernel(IgemmArgs a, int tiles_x, int tiles_y, int ntiles) {
  static_assert(!(F16 && GN), "the fused GroupNorm statistics are an encoder (bf16) feature");
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
  // input GroupNorm + lrelu (a.in_gn; the 64-channel instances only -- the 32-channel ones run at 4 waves per SIMD
  // and would spill the 32 extra VGPRs): 512 % 8 == 0, so a thread's pieces all hold channels (tid % 8) * 8 .. +7,
  // whose (mean, scale, shift) are loaded once per tile
  constexpr bool kGnIn = CINP == 64;
  float4 gnp[8];
  uint32_t inimg = 0;
  auto fetch = [&](int t) {
    const int tx = t % tiles_x;
    const int t2 = t / tiles_x;
    const int ty = t2 % tiles_y;
    const int nn = t2 / tiles_y;
    const int y0 = ty * TH - a.pad, x0 = tx * C::TW - a.pad;
    inimg = 0;
#pragma unroll
    for (int k = 0; k < C::PER_T; ++k) {
      const int e = tid + 512 * k;
      const int pi = e / (CINP / 8), part = e - pi * (CINP / 8);
      const int hr = pi / C::HC, hc = pi - hr * C::HC;
      const int iy = y0 + hr, ix = x0 + hc;
      const bool ok = e < C::NPIECE && (unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w_;
      inimg |= (uint32_t)ok << k;
      pre[k] = ok ? *reinterpret_cast<const uint4*>(xg + ((((int64_t)nn * a.h + iy) * a.w_ + ix) * CINP + part * 8) * 2)
                  : make_uint4(0u, 0u, 0u, 0u);
    }
    if constexpr (kGnIn) {
      if (a.in_gn) {
        const float4* tb = reinterpret_cast<const float4*>(a.in_gn) + ((int64_t)nn * CINP + (tid % (CINP / 8)) * 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) gnp[c] = tb[c];
      }
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
        uint4 v = pre[k];
        if constexpr (kGnIn) {  // zero padding stays zero: only in-image pieces are normalised
          if (a.in_gn && ((inimg >> k) & 1u)) v = gn_lrelu_bf16x8(v, gnp, a.in_slope);
        }
        *reinterpret_cast<uint4*>(halo + pi * C::PPB + part * 16) = v;
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
    // GN (fused statistics, groups = 32 over all COUTP channels): CPG = COUTP / 32 channels per group, so a
    // lane's 4 channels 16i + 4fh .. +3 fall in 4 / CPG groups
    constexpr int CPG = COUTP / 32, GL = 4 / CPG;
    float gs[C::OB][GL], gq[C::OB][GL];
    if constexpr (GN) {
#pragma unroll
      for (int i = 0; i < C::OB; ++i)
#pragma unroll
        for (int r = 0; r < GL; ++r) gs[i][r] = gq[i][r] = 0.f;
    }
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
        if constexpr (GN) {  // statistics of the value as stored: bias added, rounded to bf16
          const float bv[4] = {bi[i].x, bi[i].y, bi[i].z, bi[i].w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float st = bf2f(f2bf(v[r] + bv[r]));
            gs[i][r / CPG] += st;
            gq[i][r / CPG] += st * st;
          }
        }
      }
    }
    if constexpr (GN) {
      // wave: sum over the 16 pixel lanes; workgroup: 8 waves through LDS (the halo region, after a barrier);
      // then one thread per group sums the waves in a fixed order -> part[(nn, g, tile)]
#pragma unroll
      for (int i = 0; i < C::OB; ++i)
#pragma unroll
        for (int r = 0; r < GL; ++r)
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) {
            gs[i][r] += __shfl_xor(gs[i][r], off, 64);
            gq[i][r] += __shfl_xor(gq[i][r], off, 64);
          }
      __syncthreads();  // every wave is past its halo reads
      float* red = reinterpret_cast<float*>(halo);  // [2][8 waves][32 groups]
      if (fr == 0) {
#pragma unroll
        for (int i = 0; i < C::OB; ++i)
#pragma unroll
          for (int r = 0; r < GL; ++r) {
            const int g = (16 * i + 4 * fh) / CPG + r;
            red[wave * 32 + g] = gs[i][r];
            red[(8 + wave) * 32 + g] = gq[i][r];
          }
      }
      __syncthreads();
      if (tid < 32) {
        double sg = 0.0, qg = 0.0;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) {
          sg += (double)red[w8 * 32 + tid];
          qg += (double)red[(8 + w8) * 32 + tid];
        }
        double* o = a.gn_part + (((int64_t)nn * 32 + tid) * (tiles_x * tiles_y) + (ty * tiles_x + tx)) * 2;
        o[0] = sg;
        o[1] = qg;
      }
      // the next tile's first barrier orders these LDS reads before its halo stores
    }
  }
}

template <int CINP, int COUTP, bool GN, bool F16>
static void launch_hconv_t(const IgemmArgs& a, hipStream_t s) {
  constexpr int TH = CINP > 64 ? 4 : 8;  // 96 channels: 4-row tiles keep halo + weight within 160 KB of LDS
  const int tiles_x = (int)ceil_div(a.wo, 32), tiles_y = (int)ceil_div(a.ho, TH);
  const int ntiles = a.n * tiles_x * tiles_y;
  static int resident = 0;
  if (resident == 0) {
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, hconv_kernel<CINP, COUTP, TH, GN, F16>, 512, 0);
    resident = (cus > 0 ? cus : 256) * (per_cu > 0 ? per_cu : 1);
  }
  const int grid = ntiles < resident ? ntiles : resident;
  hipLaunchKernelGGL((hconv_kernel<CINP, COUTP, TH, GN, F16>), dim3((unsigned)grid), dim3(512), 0, s, a, tiles_x,
                     tiles_y, ntiles);
}
// the instance of a's cin_p in {32, 64, 96} x cout_p in {32, 64} (hconv_eligible, conv_dispatch.hip)
template <bool GN, bool F16>
static void launch_hconv_cfg(const IgemmArgs& a, hipStream_t s) {
  if (a.cin_p == 32 && a.cout_p == 32) launch_hconv_t<32, 32, GN, F16>(a, s);
  else if (a.cin_p == 32) launch_hconv_t<32, 64, GN, F16>(a, s);
  else if (a.cin_p == 64 && a.cout_p == 32) launch_hconv_t<64, 32, GN, F16>(a, s);
  else if (a.cin_p == 64) launch_hconv_t<64, 64, GN, F16>(a, s);
  else if (a.cout_p == 32) launch_hconv_t<96, 32, GN, F16>(a, s);
  else launch_hconv_t<96, 64, GN, F16>(a, s);
}
// gn_stats: the fused GroupNorm statistics (a.gn_part), bf16 only
void launch_hconv(const IgemmArgs& a, bool gn_stats, bool f16, hipStream_t s) {
  if (gn_stats) launch_hconv_cfg<true, false>(a, s);
  else if (f16) launch_hconv_cfg<false, true>(a, s);
  else launch_hconv_cfg<false, false>(a, s);
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
