// Fused uint8 PSNR + SSIM pass: one read of both images gives the per-image uint8 squared error and, per
// (image, channel), the sum of the SSIM map over the fully-inside windows (skimage structural_similarity defaults:
// uniform win x win window, sample covariance, K1 = 0.01, K2 = 0.03, data_range 255; hvae_training.py:382-395).
//
// A workgroup of 256 threads owns a tile of QT_OY x QT_OX = 32 x 64 window origins of one (image, channel):
//   1. stage the tile plus its win-1 halo of both images into LDS as converted bytes (float4 loads along W when
//      W % 4 == 0 and the bases are 16-byte aligned, dword loads otherwise); the squared error of the tile's own
//      pixels is taken from the same registers (the last tile of a row / column also owns its halo, so every
//      pixel is counted once);
//   2. horizontal win-sums of x, y, x^2, y^2, xy per staged row, four adjacent columns per thread from dword LDS
//      reads, as exact int32 (<= 11 * 255^2) into four LDS planes (sum x | sum y << 16, sum xx, sum yy, sum xy);
//   3. vertical sliding sums (a wave owns 8 origin rows, a lane one column), S in f64 from the exact integer
//      moments (<= 121 * 255^2), contraction off, summed per thread top to bottom;
//   4. fixed-order reduction over the workgroup; one partial per tile to scratch.
// A finalize kernel sums the partials per (image, channel) / per image in a fixed order: no atomics, and the result
// of an image depends on nothing but that image.
#include "common.h"

namespace ic2 {

constexpr int QT_OY = 32;       // window origins per tile, rows
constexpr int QT_OX = 64;       // window origins per tile, columns
constexpr int QT_PITCH_DW = 20; // staged row pitch in dwords (74 bytes at win 11); 45 KB of LDS at win 7: 3 per CU

struct QualityConsts {
  double inv_np, cov_norm, c1, c2;
};

// fixed-order sum over the 256 threads: xor tree inside each wave, then wave 0..3 in order; valid in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double ssim_value(int sx, int sy, int sxx, int syy, int sxy, const QualityConsts k) {
#pragma clang fp contract(off)  // identical images: 2 ux ux + C1 and ux^2 + ux^2 + C1 must round alike -> S == 1
  // means as moment * (1 / NP): one rounding more than a division (relative 1.1e-16, < 3e-13 in S through the
  // variance difference over C2), a fifth of the f64 work
  const double ux = (double)sx * k.inv_np, uy = (double)sy * k.inv_np;
  const double uxx = (double)sxx * k.inv_np, uyy = (double)syy * k.inv_np, uxy = (double)sxy * k.inv_np;
  const double vx = k.cov_norm * (uxx - ux * ux);
  const double vy = k.cov_norm * (uyy - uy * uy);
  const double vxy = k.cov_norm * (uxy - ux * uy);
  const double a1 = 2.0 * ux * uy + k.c1, a2 = 2.0 * vxy + k.c2;
  const double b1 = ux * ux + uy * uy + k.c1, b2 = vx + vy + k.c2;
  return (a1 * a2) / (b1 * b2);
}

template <int WIN, bool VEC>
__global__ void __launch_bounds__(256) uint8_quality_tile_kernel(const float* __restrict__ a,
                                                                 const float* __restrict__ b, int h, int w, int ntx,
                                                                 int nty, QualityConsts k,
                                                                 double* __restrict__ ssim_part,
                                                                 double* __restrict__ sse_part) {
  constexpr int SR = QT_OY + WIN - 1;  // staged rows
  constexpr int SC = QT_OX + WIN - 1;  // staged columns
  constexpr int SCQ = (SC + 3) / 4;    // staged float4 quads per row
  static_assert(SCQ <= QT_PITCH_DW && QT_OX / 4 + (WIN + 3 + 3) / 4 <= QT_PITCH_DW, "row pitch too short");
  __shared__ uint32_t img_a[SR * QT_PITCH_DW], img_b[SR * QT_PITCH_DW];
  __shared__ uint32_t hs[4][SR][QT_OX];
  __shared__ double red[2][4];

  const int t = threadIdx.x;
  const int nt = ntx * nty;
  const int tile = blockIdx.x % nt;
  const int64_t plane = blockIdx.x / nt;
  const int tx = tile % ntx, ty = tile / ntx;
  const int x0 = tx * QT_OX, y0 = ty * QT_OY;
  const bool last_x = tx == ntx - 1, last_y = ty == nty - 1;
  const float* pa = a + plane * h * w;
  const float* pb = b + plane * h * w;

  // ---- 1. stage both images as bytes; squared error of the pixels this tile owns
  int sq = 0;  // <= 13 pixels per thread * 255^2
  if (VEC) {
    // every quad of the thread is loaded before the first is converted, so the loads are in flight together; a quad
    // outside the image (w % 4 == 0: inside or outside as a whole) reads the zero line instead of branching
    constexpr int NQ = SR * SCQ, IT = (NQ + 255) / 256;
    float4 u[IT], v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = t + 256 * it, r = i / SCQ, q = i - r * SCQ;
      const int y = y0 + r, x = x0 + 4 * q;
      const bool inside = i < NQ && y < h && x < w;
      const int64_t off = (int64_t)y * w + x;
      u[it] = *reinterpret_cast<const float4*>(inside ? (const void*)(pa + off) : zero_line());
      v[it] = *reinterpret_cast<const float4*>(inside ? (const void*)(pb + off) : zero_line());
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = t + 256 * it, r = i / SCQ, q = i - r * SCQ;
      const bool inside = y0 + r < h && x0 + 4 * q < w;
      const int a0 = to_u8(u[it].x), a1 = to_u8(u[it].y), a2 = to_u8(u[it].z), a3 = to_u8(u[it].w);
      const int b0 = to_u8(v[it].x), b1 = to_u8(v[it].y), b2 = to_u8(v[it].z), b3 = to_u8(v[it].w);
      const uint32_t wa = (uint32_t)a0 | (uint32_t)a1 << 8 | (uint32_t)a2 << 16 | (uint32_t)a3 << 24;
      const uint32_t wb = (uint32_t)b0 | (uint32_t)b1 << 8 | (uint32_t)b2 << 16 | (uint32_t)b3 << 24;
      if (i < NQ) {
        if (inside && (r < QT_OY || last_y) && (4 * q < QT_OX || last_x))  // QT_OX % 4 == 0: the quad has one owner
          sq += (a0 - b0) * (a0 - b0) + (a1 - b1) * (a1 - b1) + (a2 - b2) * (a2 - b2) + (a3 - b3) * (a3 - b3);
        img_a[r * QT_PITCH_DW + q] = inside ? wa : 0u;
        img_b[r * QT_PITCH_DW + q] = inside ? wb : 0u;
      }
    }
  } else {
    uint8_t* ba = reinterpret_cast<uint8_t*>(img_a);
    uint8_t* bb = reinterpret_cast<uint8_t*>(img_b);
    for (int i = t; i < SR * SC; i += 256) {
      const int r = i / SC, c = i - r * SC;
      const int y = y0 + r, x = x0 + c;
      int ua = 0, ub = 0;
      if (y < h && x < w) {
        ua = to_u8(pa[(int64_t)y * w + x]);
        ub = to_u8(pb[(int64_t)y * w + x]);
        if ((r < QT_OY || last_y) && (c < QT_OX || last_x)) sq += (ua - ub) * (ua - ub);
      }
      ba[r * (QT_PITCH_DW * 4) + c] = (uint8_t)ua;
      bb[r * (QT_PITCH_DW * 4) + c] = (uint8_t)ub;
    }
  }
  __syncthreads();

  // ---- 2. horizontal win-sums: item = (staged row, group of 4 adjacent origin columns)
  constexpr int NB = WIN + 3;        // bytes a group of 4 origins reads
  constexpr int ND = (NB + 3) / 4;   // dwords holding them (the group starts dword-aligned)
  for (int i = t; i < SR * (QT_OX / 4); i += 256) {
    const int r = i >> 4, j = i & 15;
    int xa[ND * 4], xb[ND * 4];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const uint32_t wa = img_a[r * QT_PITCH_DW + j + d], wb = img_b[r * QT_PITCH_DW + j + d];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xa[4 * d + e] = (int)((wa >> (8 * e)) & 255u);
        xb[4 * d + e] = (int)((wb >> (8 * e)) & 255u);
      }
    }
    // Each origin's sums are taken directly: plain sums of byte products are what v_dot4_u32_u8 computes.  Do not
    // slide them (+ entering - leaving product): hipcc (ROCm 7.0) folds that form of sum xy into dot4 with the
    // leaving products added instead of subtracted.
    uint32_t o0[4], o1[4], o2[4], o3[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
      for (int e = 0; e < WIN; ++e) {
        const int va = xa[o + e], vb = xb[o + e];
        sx += va, sy += vb, sxx += va * va, syy += vb * vb, sxy += va * vb;
      }
      o0[o] = (uint32_t)sx | (uint32_t)sy << 16, o1[o] = (uint32_t)sxx, o2[o] = (uint32_t)syy, o3[o] = (uint32_t)sxy;
    }
    *reinterpret_cast<uint4*>(&hs[0][r][4 * j]) = make_uint4(o0[0], o0[1], o0[2], o0[3]);
    *reinterpret_cast<uint4*>(&hs[1][r][4 * j]) = make_uint4(o1[0], o1[1], o1[2], o1[3]);
    *reinterpret_cast<uint4*>(&hs[2][r][4 * j]) = make_uint4(o2[0], o2[1], o2[2], o2[3]);
    *reinterpret_cast<uint4*>(&hs[3][r][4 * j]) = make_uint4(o3[0], o3[1], o3[2], o3[3]);
  }
  __syncthreads();

  // ---- 3. vertical sliding sums and S: wave g owns origin rows 8g .. 8g+7, lane = origin column.  The packed
  // (sum x | sum y << 16) plane adds and subtracts field-wise: each field stays within [0, 121 * 255] < 2^16.
  constexpr int ROWS = QT_OY / 4;
  const int col = t & 63, r0 = (t >> 6) * ROWS;
  const bool col_ok = x0 + col + WIN <= w;
  uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
#pragma unroll
  for (int e = 0; e < WIN; ++e) {
    m0 += hs[0][r0 + e][col], m1 += hs[1][r0 + e][col], m2 += hs[2][r0 + e][col], m3 += hs[3][r0 + e][col];
  }
  double ssum = 0.0;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    if (i > 0) {
      m0 += hs[0][r0 + i + WIN - 1][col] - hs[0][r0 + i - 1][col];
      m1 += hs[1][r0 + i + WIN - 1][col] - hs[1][r0 + i - 1][col];
      m2 += hs[2][r0 + i + WIN - 1][col] - hs[2][r0 + i - 1][col];
      m3 += hs[3][r0 + i + WIN - 1][col] - hs[3][r0 + i - 1][col];
    }
    const double s = ssim_value((int)(m0 & 0xffffu), (int)(m0 >> 16), (int)m1, (int)m2, (int)m3, k);
    if (col_ok && y0 + r0 + i + WIN <= h) ssum += s;
  }

  // ---- 4. fixed-order reduction, one partial per tile
  const double tile_ssim = block_sum_256(ssum, red[0]);
  const double tile_sse = block_sum_256((double)sq, red[1]);
  if (t == 0) {
    ssim_part[blockIdx.x] = tile_ssim;
    sse_part[blockIdx.x] = tile_sse;
  }
}

// One wave per output: blocks [0, planes) sum a plane's nt SSIM partials, blocks [planes, planes + n_img) an image's
// c * nt squared-error partials.  Each lane sums its stride-64 subset in index order, then a fixed xor tree.
__global__ void __launch_bounds__(64) uint8_quality_finalize_kernel(const double* __restrict__ ssim_part,
                                                                    const double* __restrict__ sse_part,
                                                                    int64_t planes, int c, int nt,
                                                                    double* __restrict__ ssim_sum_out,
                                                                    double* __restrict__ sse_out) {
  const int64_t blk = blockIdx.x;
  const bool is_ssim = blk < planes;
  const int64_t len = is_ssim ? nt : (int64_t)c * nt;
  const double* p = is_ssim ? ssim_part + blk * nt : sse_part + (blk - planes) * len;
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < len; i += 64) v += p[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if (threadIdx.x == 0) {
    if (is_ssim)
      ssim_sum_out[blk] = v;
    else
      sse_out[blk - planes] = v;
  }
}

static int64_t quality_tiles(int h, int w, int win) {
  return ceil_div(h - win + 1, QT_OY) * ceil_div(w - win + 1, QT_OX);
}

static bool quality_shape_ok(int64_t n_img, int c, int h, int w, int win) {
  return n_img > 0 && c > 0 && h > 0 && w > 0 && win >= 3 && win <= 11 && (win & 1) && h >= win && w >= win;
}

template <int WIN>
static void launch_quality_tiles(bool vec, unsigned blocks, hipStream_t s, const float* a, const float* b, int h, int w,
                                 int ntx, int nty, const QualityConsts& k, double* ssim_part, double* sse_part) {
  if (vec)
    hipLaunchKernelGGL((uint8_quality_tile_kernel<WIN, true>), dim3(blocks), dim3(256), 0, s, a, b, h, w, ntx, nty, k,
                       ssim_part, sse_part);
  else
    hipLaunchKernelGGL((uint8_quality_tile_kernel<WIN, false>), dim3(blocks), dim3(256), 0, s, a, b, h, w, ntx, nty, k,
                       ssim_part, sse_part);
}

}  // namespace ic2

using namespace ic2;

extern "C" int64_t ic2_uint8_quality_scratch_doubles(int64_t n_img, int c, int h, int w, int win) {
  if (!quality_shape_ok(n_img, c, h, w, win)) return 0;
  return 2 * n_img * c * quality_tiles(h, w, win);
}

extern "C" int ic2_uint8_quality(const float* a, const float* b, int64_t n_img, int c, int h, int w, int win,
                                 double* sse_out, double* ssim_sum_out, double* scratch, void* stream) {
  IC2_CHECK_ARG(a && b && sse_out && ssim_sum_out && scratch,
                "uint8_quality: null pointer (a, b, sse_out, ssim_sum_out and scratch are required)");
  IC2_CHECK_ARG(n_img > 0 && c > 0 && h > 0 && w > 0, "uint8_quality: n_img=%lld c=%d h=%d w=%d must be positive",
                (long long)n_img, c, h, w);
  IC2_CHECK_ARG(win >= 3 && win <= 11 && (win & 1), "uint8_quality: win=%d must be odd and within [3, 11]", win);
  IC2_CHECK_ARG(h >= win && w >= win, "uint8_quality: win=%d exceeds the image (h=%d, w=%d)", win, h, w);
  const int64_t planes = n_img * c;
  const int ntx = (int)ceil_div(w - win + 1, QT_OX), nty = (int)ceil_div(h - win + 1, QT_OY);
  const int64_t nt = (int64_t)ntx * nty;
  IC2_CHECK_ARG(nt <= INT32_MAX && planes * nt <= INT32_MAX && planes + n_img <= INT32_MAX,
                "uint8_quality: n_img=%lld c=%d h=%d w=%d is more tiles than one launch holds", (long long)n_img, c, h,
                w);
  // skimage's constants, evaluated in double as Python evaluates (0.01 * 255) ** 2 and (0.03 * 255) ** 2
  const double np = (double)(win * win), k1r = 0.01 * 255.0, k2r = 0.03 * 255.0;
  const QualityConsts k = {1.0 / np, np / (np - 1.0), k1r * k1r, k2r * k2r};
  double* ssim_part = scratch;
  double* sse_part = scratch + planes * nt;
  const bool vec = w % 4 == 0 && ((uintptr_t)a | (uintptr_t)b) % 16 == 0;
  hipStream_t s = as_stream(stream);
  const unsigned blocks = (unsigned)(planes * nt);
  switch (win) {
    case 3: launch_quality_tiles<3>(vec, blocks, s, a, b, h, w, ntx, nty, k, ssim_part, sse_part); break;
    case 5: launch_quality_tiles<5>(vec, blocks, s, a, b, h, w, ntx, nty, k, ssim_part, sse_part); break;
    case 7: launch_quality_tiles<7>(vec, blocks, s, a, b, h, w, ntx, nty, k, ssim_part, sse_part); break;
    case 9: launch_quality_tiles<9>(vec, blocks, s, a, b, h, w, ntx, nty, k, ssim_part, sse_part); break;
    default: launch_quality_tiles<11>(vec, blocks, s, a, b, h, w, ntx, nty, k, ssim_part, sse_part); break;
  }
  hipLaunchKernelGGL(uint8_quality_finalize_kernel, dim3((unsigned)(planes + n_img)), dim3(64), 0, s, ssim_part,
                     sse_part, planes, c, (int)nt, ssim_sum_out, sse_out);
  IC2_CHECK_LAUNCH("uint8_quality");
  return IC2_OK;
}
