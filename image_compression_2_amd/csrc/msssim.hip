// MS-SSIM (five scales, 11-tap Gaussian window sigma 1.5, "valid" maps, weights in the caller): the per-(image,
// channel, scale) terms in f64 and, for the loss, the gradient of a caller-weighted sum of those terms.
//
// Working values are CENTRED: v = x * 0.5 (loss mode; the data range is 1 and the centre 0.5) or v = u - 127.5 (metric
// mode; u the reference's uint8 conversion, data range 255).  Variances and the covariance do not change under a common
// shift, so sigma^2 = g*v^2 - (g*v)^2 is formed where the cancellation is mildest; only the luminance factor of the last
// scale needs the mean itself, mu = g*v + centre.  The pooled pyramid (levels 1..4) is stored centred too: the pool's
// zero padding on an odd axis is the value -centre there.
//
// Forward, per scale: ms_ssim_scale_kernel, one workgroup of 256 per (plane, MT_Y x MT_X tile of map positions):
//   1. stage the tile plus its 10-pixel halo of both images into LDS (row pitch 43: the four rows a 32-lane half reads
//      in step 2 start on different banks mod 4);
//   2. horizontal 11-tap pass on v_x, v_y, v_x^2, v_y^2, v_x v_y, four adjacent columns per thread, into five LDS planes
//      [row][32 columns];
//   3. vertical pass: a lane owns a column and four map rows (a 32-lane half reads 32 consecutive dwords of one plane
//      row: no bank conflict), then cs and the luminance factor per position;
//   4. fixed-order f64 reduction, one partial per tile.
// ms_ssim_pool_kernel writes the next level of both images; ms_ssim_finalize_kernel sums the partials per (plane, scale)
// in a fixed order and divides by the number of map positions.  No atomics: a plane's terms depend on that plane alone.
//
// Backward, per scale from coarse to fine: ms_ssim_bwd_kernel, one workgroup per (plane, MB_Y x MB_X tile of pixels):
// stage the pixels' 20-pixel surround, recompute the five filtered images on the (MB_Y + 10) x (MB_X + 10) map positions
// whose windows touch the tile, form the adjoint maps d t / d(g*v_x), d t / d(g*v_y), d t / d(g*v_x^2) (= that of v_y^2)
// and d t / d(g*v_x v_y) scaled by gterms / positions, apply the transposed separable filter and combine
//   g_x = A_x + 2 v_x B + v_y C,   g_y = A_y + 2 v_y B + v_x C,
// add a quarter of the next-coarser level's gradient at the pixel's pool cell, and store the level's gradient plane
// (level 0: times 0.5, into the caller's ga / gb).  With one of ga / gb NULL its A map is neither written nor filtered.
#include "common.h"

namespace ic2 {

constexpr int MS_TAPS = 11, MS_HALO = MS_TAPS - 1, MS_LEVELS = 5;
constexpr int MS_MIN_SIDE = MS_HALO * 16 + 1;  // 161: the last scale is at least one window

constexpr int MT_Y = 32, MT_X = 32;                      // forward: map positions per tile (metrics.MS_SSIM_TILE)
constexpr int MT_SR = MT_Y + MS_HALO, MT_SC = MT_X + MS_HALO;
constexpr int MT_PITCH = MT_SC + 1;                      // 43 dwords
// forward LDS: 2 * 42 * 43 * 4 + 5 * 42 * 32 * 4 = 41.3 KB: three workgroups per CU

constexpr int MB_Y = 16, MB_X = 32;                      // backward: pixels per tile
constexpr int MB_MR = MB_Y + MS_HALO;                    // 26 map rows
constexpr int MB_MC = 44;                                // 42 map columns, padded to whole quads
constexpr int MB_SR = MB_MR + MS_HALO;                   // 36 staged rows
constexpr int MB_SC = MB_MC + MS_HALO;                   // 54 staged columns
constexpr int MB_PITCH = MB_SC + 1;                      // 55 dwords (3 mod 4, as the forward's)
constexpr int MB_AC = MB_X + MS_HALO;                   // 42 adjoint-map columns kept
// backward LDS: 2 * 36 * 55 * 4 + 5 * 36 * 44 * 4 + 4 * 26 * 42 * 4 = 63.5 KB: two workgroups per CU

struct MsWindow {
  float g[MS_TAPS];
};

struct MsConsts {
  float centre, c1, c2;
};

enum { MS_SRC_LOSS = 0, MS_SRC_METRIC = 1, MS_SRC_LEVEL = 2 };

// a level-0 input or a stored pyramid value -> the centred working value
template <int SRC>
__device__ __forceinline__ float ms_value(float v) {
  if (SRC == MS_SRC_LOSS) return v * 0.5f;
  if (SRC == MS_SRC_METRIC) return (float)to_u8(v) - 127.5f;
  return v;
}

// fixed-order sum over 256 threads: xor tree inside each wave, then waves 0..3 in order; valid in thread 0
__device__ __forceinline__ double ms_block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// cs and the luminance factor of one map position.  Identical images: exy, exx and eyy were formed by the same
// operations on the same values, so sxy == sxx == syy and 2 sxy + C2 == (sxx + syy) + C2 bit for bit; likewise
// 2 (ux uy) + C1 == (ux ux + uy uy) + C1 with every product rounded on its own (no contraction).
__device__ __forceinline__ void ms_point(float mx, float my, float exx, float eyy, float exy, const MsConsts k,
                                         float& cs, float& lum) {
#pragma clang fp contract(off)
  const float pxx = mx * mx, pyy = my * my, pxy = mx * my;
  const float sxx = exx - pxx, syy = eyy - pyy, sxy = exy - pxy;
  cs = (2.f * sxy + k.c2) / ((sxx + syy) + k.c2);
  const float ux = mx + k.centre, uy = my + k.centre;
  const float qxx = ux * ux, qyy = uy * uy, qxy = ux * uy;
  lum = (2.f * qxy + k.c1) / ((qxx + qyy) + k.c1);
}

// four adjacent outputs of the 11-tap filter over 14 values
__device__ __forceinline__ float4 ms_fir4(const float* v, const MsWindow& win) {
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
#pragma unroll
  for (int e = 0; e < MS_TAPS; ++e) {
    o0 = fmaf(win.g[e], v[e], o0);
    o1 = fmaf(win.g[e], v[e + 1], o1);
    o2 = fmaf(win.g[e], v[e + 2], o2);
    o3 = fmaf(win.g[e], v[e + 3], o3);
  }
  return make_float4(o0, o1, o2, o3);
}

// horizontal pass of one (staged row, quad of columns): the five filtered rows of x, y, x^2, y^2, xy
__device__ __forceinline__ void ms_hpass_quad(const float* ra, const float* rb, const MsWindow& win, float4 out[5]) {
  float xa[MS_TAPS + 3], xb[MS_TAPS + 3], p[MS_TAPS + 3];
#pragma unroll
  for (int e = 0; e < MS_TAPS + 3; ++e) xa[e] = ra[e], xb[e] = rb[e];
  out[0] = ms_fir4(xa, win);
  out[1] = ms_fir4(xb, win);
#pragma unroll
  for (int e = 0; e < MS_TAPS + 3; ++e) p[e] = xa[e] * xa[e];
  out[2] = ms_fir4(p, win);
#pragma unroll
  for (int e = 0; e < MS_TAPS + 3; ++e) p[e] = xb[e] * xb[e];
  out[3] = ms_fir4(p, win);
#pragma unroll
  for (int e = 0; e < MS_TAPS + 3; ++e) p[e] = xa[e] * xb[e];
  out[4] = ms_fir4(p, win);
}

template <int SRC>
__global__ void __launch_bounds__(256) ms_ssim_scale_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            int h, int w, int ntx, int nty, MsWindow win, MsConsts k,
                                                            int use_lum, double* __restrict__ part) {
  __shared__ float sa[MT_SR * MT_PITCH], sb[MT_SR * MT_PITCH];
  __shared__ __attribute__((aligned(16))) float hs[5][MT_SR][MT_X];
  __shared__ double red[4];

  const int t = threadIdx.x;
  const int nt = ntx * nty;
  const int tile = blockIdx.x % nt;
  const int64_t plane = blockIdx.x / nt;
  const int tx = tile % ntx, ty = tile / ntx;
  const int x0 = tx * MT_X, y0 = ty * MT_Y;
  const float* pa = a + plane * h * w;
  const float* pb = b + plane * h * w;

  // ---- 1. stage: every load issued before the first conversion; outside the image the zero line is read
  {
    constexpr int NE = MT_SR * MT_SC, IT = (NE + 255) / 256;
    float u[IT], v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = t + 256 * it, r = i / MT_SC, c = i - r * MT_SC;
      const int y = y0 + r, x = x0 + c;
      const bool inside = i < NE && y < h && x < w;
      const int64_t off = (int64_t)y * w + x;
      u[it] = *(inside ? pa + off : reinterpret_cast<const float*>(zero_line()));
      v[it] = *(inside ? pb + off : reinterpret_cast<const float*>(zero_line()));
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = t + 256 * it, r = i / MT_SC, c = i - r * MT_SC;
      if (i < NE) {
        sa[r * MT_PITCH + c] = ms_value<SRC>(u[it]);
        sb[r * MT_PITCH + c] = ms_value<SRC>(v[it]);
      }
    }
  }
  __syncthreads();

  // ---- 2. horizontal pass
  for (int i = t; i < MT_SR * (MT_X / 4); i += 256) {
    const int r = i >> 3, q = i & 7;
    float4 o[5];
    ms_hpass_quad(&sa[r * MT_PITCH + 4 * q], &sb[r * MT_PITCH + 4 * q], win, o);
#pragma unroll
    for (int p = 0; p < 5; ++p) *reinterpret_cast<float4*>(&hs[p][r][4 * q]) = o[p];
  }
  __syncthreads();

  // ---- 3. vertical pass: lane = column, four map rows per thread
  constexpr int ROWS = MT_Y / 8;
  const int col = t & 31, r0 = (t >> 5) * ROWS;
  float f[5][ROWS];
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    float v[ROWS + MS_HALO];
#pragma unroll
    for (int e = 0; e < ROWS + MS_HALO; ++e) v[e] = hs[p][r0 + e][col];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < MS_TAPS; ++e) acc = fmaf(win.g[e], v[i + e], acc);
      f[p][i] = acc;
    }
  }
  const bool col_ok = x0 + col + MS_HALO < w;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    float cs, lum;
    ms_point(f[0][i], f[1][i], f[2][i], f[3][i], f[4][i], k, cs, lum);
    const float val = use_lum ? lum * cs : cs;
    if (col_ok && y0 + r0 + i + MS_HALO < h) sum += (double)val;
  }

  // ---- 4. one partial per tile
  const double tile_sum = ms_block_sum(sum, red);
  if (t == 0) part[blockIdx.x] = tile_sum;
}

// Next level of both images: 2 x 2 mean, stride 2; an odd axis is padded by one zero (centred: -centre) at both ends, so
// output i covers inputs 2i-1 and 2i there.
template <int SRC>
__global__ void __launch_bounds__(256) ms_ssim_pool_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           int h, int w, int h1, int w1, int64_t total, float centre,
                                                           float* __restrict__ oa, float* __restrict__ ob) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t hw1 = (int64_t)h1 * w1;
  const int64_t plane = idx / hw1;
  const int rem = (int)(idx - plane * hw1);
  const int i = rem / w1, j = rem - i * w1;
  const int ya = 2 * i - (h & 1), xa = 2 * j - (w & 1);
  const float* pa = a + plane * h * w;
  const float* pb = b + plane * h * w;
  float va[4], vb[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int y = ya + (d >> 1), x = xa + (d & 1);
    const bool inside = y >= 0 && y < h && x >= 0 && x < w;
    va[d] = inside ? ms_value<SRC>(pa[(int64_t)y * w + x]) : -centre;
    vb[d] = inside ? ms_value<SRC>(pb[(int64_t)y * w + x]) : -centre;
  }
  oa[idx] = ((va[0] + va[1]) + (va[2] + va[3])) * 0.25f;
  ob[idx] = ((vb[0] + vb[1]) + (vb[2] + vb[3])) * 0.25f;
}

struct MsFinalize {
  int64_t part_off[MS_LEVELS];  // first partial of a scale
  int nt[MS_LEVELS];            // tiles per plane
  double count[MS_LEVELS];      // map positions per plane
};

// One wave per (plane, scale): each lane sums its stride-64 subset of the plane's partials in index order, then a fixed
// xor tree; the mean is a division by the count (identical images: count / count == 1.0).
__global__ void __launch_bounds__(64) ms_ssim_finalize_kernel(const double* __restrict__ part, MsFinalize fz,
                                                              double* __restrict__ terms) {
  const int64_t plane = blockIdx.x / MS_LEVELS;
  const int s = blockIdx.x % MS_LEVELS;
  const int nt = fz.nt[s];
  const double* p = part + fz.part_off[s] + plane * nt;
  double v = 0.0;
  for (int i = threadIdx.x; i < nt; i += 64) v += p[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if (threadIdx.x == 0) terms[blockIdx.x] = v / fz.count[s];
}

template <int SRC>
__global__ void __launch_bounds__(256) ms_ssim_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          int h, int w, int ntx, int nty, MsWindow win, MsConsts k,
                                                          int use_lum, const double* __restrict__ gterms, int level,
                                                          double inv_count, const float* __restrict__ next_a,
                                                          const float* __restrict__ next_b, int h1, int w1,
                                                          float out_scale, float* __restrict__ out_a,
                                                          float* __restrict__ out_b) {
  __shared__ float sa[MB_SR * MB_PITCH], sb[MB_SR * MB_PITCH];
  __shared__ __attribute__((aligned(16))) float hs[5 * MB_SR * MB_MC];   // the five horizontal-pass planes; later the four half-filtered adjoints
  __shared__ float adj[4][MB_MR][MB_AC];    // A_x, A_y, B, C

  const int t = threadIdx.x;
  const int nt = ntx * nty;
  const int tile = blockIdx.x % nt;
  const int64_t plane = blockIdx.x / nt;
  const int tx = tile % ntx, ty = tile / ntx;
  const int x0 = tx * MB_X, y0 = ty * MB_Y;        // first pixel of the tile
  const int sx0 = x0 - MS_HALO, sy0 = y0 - MS_HALO;  // first staged pixel = first map position
  const float* pa = a + plane * h * w;
  const float* pb = b + plane * h * w;
  const float scale = (float)(gterms[plane * MS_LEVELS + level] * inv_count);

  // ---- 1. stage the 36 x 54 surround
  {
    constexpr int NE = MB_SR * MB_SC, IT = (NE + 255) / 256;
    float u[IT], v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = t + 256 * it, r = i / MB_SC, c = i - r * MB_SC;
      const int y = sy0 + r, x = sx0 + c;
      const bool inside = i < NE && y >= 0 && y < h && x >= 0 && x < w;
      const int64_t off = (int64_t)y * w + x;
      u[it] = *(inside ? pa + off : reinterpret_cast<const float*>(zero_line()));
      v[it] = *(inside ? pb + off : reinterpret_cast<const float*>(zero_line()));
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = t + 256 * it, r = i / MB_SC, c = i - r * MB_SC;
      if (i < NE) {
        sa[r * MB_PITCH + c] = ms_value<SRC>(u[it]);
        sb[r * MB_PITCH + c] = ms_value<SRC>(v[it]);
      }
    }
  }
  __syncthreads();

  // ---- 2. horizontal pass over the 36 staged rows x 44 map columns
  for (int i = t; i < MB_SR * (MB_MC / 4); i += 256) {
    const int r = i / (MB_MC / 4), q = i - r * (MB_MC / 4);
    float4 o[5];
    ms_hpass_quad(&sa[r * MB_PITCH + 4 * q], &sb[r * MB_PITCH + 4 * q], win, o);
#pragma unroll
    for (int p = 0; p < 5; ++p) *reinterpret_cast<float4*>(&hs[(p * MB_SR + r) * MB_MC + 4 * q]) = o[p];
  }
  __syncthreads();

  // ---- 3. vertical pass and the adjoint maps: item = (map column, pair of map rows)
  const int mh = h - MS_HALO, mw = w - MS_HALO;
  for (int i = t; i < (MB_MR / 2) * MB_MC; i += 256) {
    const int rg = i / MB_MC, col = i - rg * MB_MC, r0 = 2 * rg;
    float f[5][2];
#pragma unroll
    for (int p = 0; p < 5; ++p) {
      float v[2 + MS_HALO];
#pragma unroll
      for (int e = 0; e < 2 + MS_HALO; ++e) v[e] = hs[(p * MB_SR + r0 + e) * MB_MC + col];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < MS_TAPS; ++e) acc = fmaf(win.g[e], v[j + e], acc);
        f[p][j] = acc;
      }
    }
    const int qx = sx0 + col;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qy = sy0 + r0 + j;
      const bool valid = qx >= 0 && qx < mw && qy >= 0 && qy < mh;
      const float mx = f[0][j], my = f[1][j];
      float cs, lum;
      ms_point(mx, my, f[2][j], f[3][j], f[4][j], k, cs, lum);
      const float sxx = f[2][j] - mx * mx, syy = f[3][j] - my * my;
      const float inv_d = 1.f / ((sxx + syy) + k.c2);
      // d cs / d(g*xy) = 2 / D;  d cs / d(g*x^2) = -cs / D;  d cs / d(g*x) = 2 (cs mx - my) / D
      float ax = 2.f * inv_d * (cs * mx - my), ay = 2.f * inv_d * (cs * my - mx);
      float bb = -cs * inv_d, cc = 2.f * inv_d;
      if (use_lum) {
        const float ux = mx + k.centre, uy = my + k.centre;
        const float inv_dl = 1.f / ((ux * ux + uy * uy) + k.c1);
        // d lum / d ux = 2 (uy - lum ux) / Dl
        ax = cs * (2.f * inv_dl * (uy - lum * ux)) + lum * ax;
        ay = cs * (2.f * inv_dl * (ux - lum * uy)) + lum * ay;
        bb *= lum, cc *= lum;
      }
      if (col >= MB_AC) continue;   // the quad padding: no pixel of the tile reads it
      if (out_a) adj[0][r0 + j][col] = valid ? scale * ax : 0.f;
      if (out_b) adj[1][r0 + j][col] = valid ? scale * ay : 0.f;
      adj[2][r0 + j][col] = valid ? scale * bb : 0.f;
      adj[3][r0 + j][col] = valid ? scale * cc : 0.f;
    }
  }
  __syncthreads();

  // ---- 4. transposed horizontal pass (the window is symmetric): pixel column px sums map columns px .. px + 10
  // Only the planes a requested gradient reads: B and C always, A_x for ga, A_y for gb.
  float* ht = hs;  // [4][MB_MR][MB_X]
  const int n_m = (out_a && out_b) ? 4 : 3;
  for (int i = t; i < n_m * MB_MR * (MB_X / 4); i += 256) {
    const int mi = i / (MB_MR * (MB_X / 4)), rq = i - mi * (MB_MR * (MB_X / 4));
    const int m = n_m == 4 ? mi : (mi == 0 ? (out_a ? 0 : 1) : mi + 1);
    const int r = rq >> 3, q = rq & 7;
    float v[MS_TAPS + 3];
#pragma unroll
    for (int e = 0; e < MS_TAPS + 3; ++e) v[e] = adj[m][r][4 * q + e];
    *reinterpret_cast<float4*>(&ht[(m * MB_MR + r) * MB_X + 4 * q]) = ms_fir4(v, win);
  }
  __syncthreads();

  // ---- 5. transposed vertical pass, combination, pool adjoint, store: lane = pixel column, two pixel rows per thread
  const int px = t & 31, py0 = (t >> 5) * 2;
  float g4[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    g4[m][0] = g4[m][1] = 0.f;
    if ((m == 0 && !out_a) || (m == 1 && !out_b)) continue;
    float v[2 + MS_HALO];
#pragma unroll
    for (int e = 0; e < 2 + MS_HALO; ++e) v[e] = ht[(m * MB_MR + py0 + e) * MB_X + px];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < MS_TAPS; ++e) acc = fmaf(win.g[e], v[j + e], acc);
      g4[m][j] = acc;
    }
  }
  const int x = x0 + px;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int y = y0 + py0 + j;
    if (x >= w || y >= h) continue;
    const float vx = sa[(py0 + j + MS_HALO) * MB_PITCH + px + MS_HALO];
    const float vy = sb[(py0 + j + MS_HALO) * MB_PITCH + px + MS_HALO];
    const int64_t o = plane * h * w + (int64_t)y * w + x;
    // the pool cell of this pixel: (y + 1) / 2 on an odd axis, y / 2 on an even one
    const int64_t on = plane * h1 * w1 + (int64_t)((y + (h & 1)) >> 1) * w1 + ((x + (w & 1)) >> 1);
    if (out_a) {
      float g = g4[0][j] + 2.f * vx * g4[2][j] + vy * g4[3][j];
      if (next_a) g += 0.25f * next_a[on];
      out_a[o] = g * out_scale;
    }
    if (out_b) {
      float g = g4[1][j] + 2.f * vy * g4[2][j] + vx * g4[3][j];
      if (next_b) g += 0.25f * next_b[on];
      out_b[o] = g * out_scale;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct MsGeom {
  int h[MS_LEVELS], w[MS_LEVELS];
  int64_t lvl_off[MS_LEVELS];   // floats before level s (1..4) in one image's pyramid of all planes
  int64_t pyr_floats;           // one image's pyramid, levels 1..4, all planes
  int ntx[MS_LEVELS], nty[MS_LEVELS];
  int64_t part_off[MS_LEVELS];  // partials before scale s
  int64_t parts;                // partials of all scales, all planes
  int64_t max_blocks;           // largest grid of any launch
};

static bool ms_shape_ok(int64_t n, int c, int h, int w) {
  return n > 0 && c > 0 && h >= MS_MIN_SIDE && w >= MS_MIN_SIDE;
}

static MsGeom ms_geom(int64_t planes, int h, int w) {
  MsGeom g;
  int64_t px = 0, parts = 0, mb = 0;
  for (int s = 0; s < MS_LEVELS; ++s) {
    g.h[s] = s ? (g.h[s - 1] + 1) / 2 : h;
    g.w[s] = s ? (g.w[s - 1] + 1) / 2 : w;
    g.lvl_off[s] = planes * px;
    if (s) px += (int64_t)g.h[s] * g.w[s];
    g.ntx[s] = (int)ceil_div(g.w[s] - MS_HALO, MT_X);
    g.nty[s] = (int)ceil_div(g.h[s] - MS_HALO, MT_Y);
    g.part_off[s] = parts;
    parts += planes * g.ntx[s] * g.nty[s];
    const int64_t fwd = planes * g.ntx[s] * g.nty[s];
    const int64_t bwd = planes * ceil_div(g.w[s], MB_X) * ceil_div(g.h[s], MB_Y);
    const int64_t pool = ceil_div(planes * g.h[s] * g.w[s], 256);
    mb = fwd > mb ? fwd : mb, mb = bwd > mb ? bwd : mb, mb = pool > mb ? pool : mb;
  }
  g.pyr_floats = planes * px;
  g.parts = parts;
  g.max_blocks = mb;
  return g;
}

static MsWindow ms_window() {
  double gd[MS_TAPS], sum = 0.0;
  for (int i = 0; i < MS_TAPS; ++i) sum += gd[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
  MsWindow win;
  for (int i = 0; i < MS_TAPS; ++i) win.g[i] = (float)(gd[i] / sum);
  return win;
}

static MsConsts ms_consts(int mode) {
  const double range = mode == IC2_MS_SSIM_METRIC ? 255.0 : 1.0;
  const double k1r = 0.01 * range, k2r = 0.03 * range;
  return {(float)(0.5 * range), (float)(k1r * k1r), (float)(k2r * k2r)};
}

static int ms_check_shape(const char* who, int64_t n, int c, int h, int w) {
  IC2_CHECK_ARG(n > 0 && c > 0 && h > 0 && w > 0, "%s: n=%lld c=%d h=%d w=%d must be positive", who, (long long)n, c, h,
                w);
  IC2_CHECK_ARG(h >= MS_MIN_SIDE && w >= MS_MIN_SIDE,
                "%s: h=%d w=%d: the smaller side must exceed (11 - 1) * 2^4 = 160 for five scales", who, h, w);
  IC2_CHECK_ARG(n * c <= INT32_MAX / MS_LEVELS && ms_geom(n * c, h, w).max_blocks <= INT32_MAX,
                "%s: n=%lld c=%d h=%d w=%d is more tiles than one launch holds", who, (long long)n, c, h, w);
  return IC2_OK;
}

}  // namespace ic2

using namespace ic2;

extern "C" int64_t ic2_ms_ssim_ws_floats(int64_t n, int c, int h, int w) {
  if (!ms_shape_ok(n, c, h, w)) return 0;
  const MsGeom g = ms_geom(n * c, h, w);
  return 2 * g.parts + 2 * g.pyr_floats;
}

extern "C" int64_t ic2_ms_ssim_bwd_ws_floats(int64_t n, int c, int h, int w) {
  if (!ms_shape_ok(n, c, h, w)) return 0;
  return 2 * ms_geom(n * c, h, w).pyr_floats;
}

extern "C" int ic2_ms_ssim_fwd(const float* a, const float* b, int mode, int64_t n, int c, int h, int w, double* terms,
                               float* ws, void* stream) {
  IC2_CHECK_ARG(a && b && terms && ws, "ms_ssim_fwd: null pointer (a, b, terms and ws are required)");
  IC2_CHECK_ARG(mode == IC2_MS_SSIM_LOSS || mode == IC2_MS_SSIM_METRIC, "ms_ssim_fwd: mode=%d must be 0 (loss) or 1 "
                "(metric)", mode);
  if (int rc = ms_check_shape("ms_ssim_fwd", n, c, h, w)) return rc;
  IC2_CHECK_ARG((uintptr_t)ws % 8 == 0, "ms_ssim_fwd: ws must be 8-byte aligned (it holds the f64 partials)");
  const int64_t planes = n * c;
  const MsGeom g = ms_geom(planes, h, w);
  const MsWindow win = ms_window();
  const MsConsts k = ms_consts(mode);
  double* part = reinterpret_cast<double*>(ws);
  float* pyr_a = ws + 2 * g.parts;
  float* pyr_b = pyr_a + g.pyr_floats;
  hipStream_t s = as_stream(stream);
  MsFinalize fz;
  for (int l = 0; l < MS_LEVELS; ++l) {
    const float* la = l ? pyr_a + g.lvl_off[l] : a;
    const float* lb = l ? pyr_b + g.lvl_off[l] : b;
    const int nt = g.ntx[l] * g.nty[l];
    const unsigned blocks = (unsigned)(planes * nt);
    double* lp = part + g.part_off[l];
    const int use_lum = l == MS_LEVELS - 1;
    if (l)
      hipLaunchKernelGGL((ms_ssim_scale_kernel<MS_SRC_LEVEL>), dim3(blocks), dim3(256), 0, s, la, lb, g.h[l], g.w[l],
                         g.ntx[l], g.nty[l], win, k, use_lum, lp);
    else if (mode == IC2_MS_SSIM_METRIC)
      hipLaunchKernelGGL((ms_ssim_scale_kernel<MS_SRC_METRIC>), dim3(blocks), dim3(256), 0, s, la, lb, g.h[l], g.w[l],
                         g.ntx[l], g.nty[l], win, k, use_lum, lp);
    else
      hipLaunchKernelGGL((ms_ssim_scale_kernel<MS_SRC_LOSS>), dim3(blocks), dim3(256), 0, s, la, lb, g.h[l], g.w[l],
                         g.ntx[l], g.nty[l], win, k, use_lum, lp);
    fz.part_off[l] = g.part_off[l];
    fz.nt[l] = nt;
    fz.count[l] = (double)(g.h[l] - MS_HALO) * (double)(g.w[l] - MS_HALO);
    if (l + 1 < MS_LEVELS) {
      const int64_t total = planes * g.h[l + 1] * g.w[l + 1];
      const unsigned pb = (unsigned)ceil_div(total, 256);
      float* oa = pyr_a + g.lvl_off[l + 1];
      float* ob = pyr_b + g.lvl_off[l + 1];
      if (l)
        hipLaunchKernelGGL((ms_ssim_pool_kernel<MS_SRC_LEVEL>), dim3(pb), dim3(256), 0, s, la, lb, g.h[l], g.w[l],
                           g.h[l + 1], g.w[l + 1], total, k.centre, oa, ob);
      else if (mode == IC2_MS_SSIM_METRIC)
        hipLaunchKernelGGL((ms_ssim_pool_kernel<MS_SRC_METRIC>), dim3(pb), dim3(256), 0, s, la, lb, g.h[l], g.w[l],
                           g.h[l + 1], g.w[l + 1], total, k.centre, oa, ob);
      else
        hipLaunchKernelGGL((ms_ssim_pool_kernel<MS_SRC_LOSS>), dim3(pb), dim3(256), 0, s, la, lb, g.h[l], g.w[l],
                           g.h[l + 1], g.w[l + 1], total, k.centre, oa, ob);
    }
  }
  hipLaunchKernelGGL(ms_ssim_finalize_kernel, dim3((unsigned)(planes * MS_LEVELS)), dim3(64), 0, s, part, fz, terms);
  IC2_CHECK_LAUNCH("ms_ssim_fwd");
  return IC2_OK;
}

extern "C" int ic2_ms_ssim_bwd(const float* a, const float* b, int mode, const float* ws_fwd, const double* gterms,
                               int64_t n, int c, int h, int w, float* ga, float* gb, float* ws_grad, void* stream) {
  if (mode == IC2_MS_SSIM_METRIC) {
    set_error("ms_ssim_bwd: metric mode has no backward (the uint8 truncation has zero gradient); use mode 0 (loss)");
    return IC2_E_UNSUPPORTED;
  }
  IC2_CHECK_ARG(mode == IC2_MS_SSIM_LOSS, "ms_ssim_bwd: mode=%d must be 0 (loss)", mode);
  IC2_CHECK_ARG(a && b && ws_fwd && gterms && ws_grad,
                "ms_ssim_bwd: null pointer (a, b, ws_fwd, gterms and ws_grad are required)");
  IC2_CHECK_ARG(ga || gb, "ms_ssim_bwd: null pointer (one of ga and gb is required)");
  if (int rc = ms_check_shape("ms_ssim_bwd", n, c, h, w)) return rc;
  const int64_t planes = n * c;
  const MsGeom g = ms_geom(planes, h, w);
  const MsWindow win = ms_window();
  const MsConsts k = ms_consts(mode);
  const float* pyr_a = ws_fwd + 2 * g.parts;
  const float* pyr_b = pyr_a + g.pyr_floats;
  float* gpyr_a = ws_grad;
  float* gpyr_b = ws_grad + g.pyr_floats;
  hipStream_t s = as_stream(stream);
  for (int l = MS_LEVELS - 1; l >= 0; --l) {
    const float* la = l ? pyr_a + g.lvl_off[l] : a;
    const float* lb = l ? pyr_b + g.lvl_off[l] : b;
    const bool last = l == MS_LEVELS - 1;
    const float* na = (ga && !last) ? gpyr_a + g.lvl_off[l + 1] : nullptr;
    const float* nb = (gb && !last) ? gpyr_b + g.lvl_off[l + 1] : nullptr;
    float* oa = ga ? (l ? gpyr_a + g.lvl_off[l] : ga) : nullptr;
    float* ob = gb ? (l ? gpyr_b + g.lvl_off[l] : gb) : nullptr;
    const int ntx = (int)ceil_div(g.w[l], MB_X), nty = (int)ceil_div(g.h[l], MB_Y);
    const unsigned blocks = (unsigned)(planes * ntx * nty);
    const double inv_count = 1.0 / ((double)(g.h[l] - MS_HALO) * (double)(g.w[l] - MS_HALO));
    const int h1 = last ? 0 : g.h[l + 1], w1 = last ? 0 : g.w[l + 1];
    if (l)
      hipLaunchKernelGGL((ms_ssim_bwd_kernel<MS_SRC_LEVEL>), dim3(blocks), dim3(256), 0, s, la, lb, g.h[l], g.w[l], ntx,
                         nty, win, k, (int)last, gterms, l, inv_count, na, nb, h1, w1, 1.f, oa, ob);
    else
      hipLaunchKernelGGL((ms_ssim_bwd_kernel<MS_SRC_LOSS>), dim3(blocks), dim3(256), 0, s, la, lb, g.h[l], g.w[l], ntx,
                         nty, win, k, (int)last, gterms, l, inv_count, na, nb, h1, w1, 0.5f, oa, ob);
  }
  IC2_CHECK_LAUNCH("ms_ssim_bwd");
  return IC2_OK;
}
