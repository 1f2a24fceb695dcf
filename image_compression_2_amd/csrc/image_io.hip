// Device-side image I/O: Pillow's 8-bit resampler (Image.resize on "L" / "RGB"), ToTensor + Normalize as a table, and
// the three f32 -> uint8 conversions of the reference's snippets.
//
// The resampler is integer arithmetic on fixed-point coefficients (22 fraction bits), so it is restated bit for bit:
//   host:   ic2_resample_coeffs builds one axis' table, (xmin, taps) and the taps' int32 coefficients per output;
//   pass 1: filters along x the source rows the vertical pass reads, uint8 into the caller's workspace;
//   pass 2: filters along y, uint8 HWC out or, through a [c][256] f32 table, f32 NCHW out.
// acc = 2^21 + sum p * k in int32 (Pillow's own accumulator; 2^21 + 255 * sum |k| stays below 2^31 for every scale
// the tables are built for), then clip(acc >> 22, 0, 255).  An axis that keeps its size gets the identity table
// (one tap of 2^22), which is exact, so the kernels have one code path.  A batch is ragged: a device record per image
// names its source, tables and workspace slice.  Threads run along output x; a row's y coefficients are uniform over
// the workgroup.  No LDS, no atomics: deterministic and capturable.
#include <cmath>
#include <vector>
#include "common.h"

namespace ic2 {

constexpr int RS_PRECISION_BITS = 22;
constexpr int RS_REC = 9;         // int64 per image record
constexpr int RS_ROWS = 4;        // source rows per thread in pass 1 (one coefficient load serves all of them)
constexpr int RS_MAX_SIZE = 16384;

// ---------------------------------------------------------------------------------------------- tables (host)
static double rs_sinc(double x) {
#pragma clang fp contract(off)
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

static double rs_filter(int filter, double x) {
#pragma clang fp contract(off)
  if (filter == IC2_RESAMPLE_BILINEAR) {
    x = fabs(x);
    return x < 1.0 ? 1.0 - x : 0.0;
  }
  if (filter == IC2_RESAMPLE_BICUBIC) {  // Keys, a = -0.5
    const double a = -0.5;
    x = fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
  }
  return (-3.0 <= x && x < 3.0) ? rs_sinc(x) * rs_sinc(x / 3.0) : 0.0;
}

static bool rs_axis_ok(int in, int out, int filter) {
  return in > 0 && in <= RS_MAX_SIZE && out > 0 && out <= RS_MAX_SIZE && filter >= IC2_RESAMPLE_BILINEAR &&
         filter <= IC2_RESAMPLE_LANCZOS;
}

static double rs_filter_support(int filter) {
  return filter == IC2_RESAMPLE_BILINEAR ? 1.0 : filter == IC2_RESAMPLE_BICUBIC ? 2.0 : 3.0;
}

// ---------------------------------------------------------------------------------------------- resample kernels
struct RsImage {
  int64_t src_off, ws_off;           // bytes into the source blob / the workspace
  const int32_t *xb, *xk, *yb, *yk;  // bounds [out][2] and coefficients [out][ksize] of the two axes
  int h, w, kx, ky, y0, rows;
};

// record: {src_off, h, w, x table, y table (int32 offsets into tables), kx, ky, ws_off, y0}
__device__ __forceinline__ RsImage rs_image(const int64_t* recs, const int32_t* tables, int img, int oh, int ow) {
  const int64_t* r = recs + (int64_t)RS_REC * img;
  RsImage I;
  I.src_off = r[0];
  I.h = (int)r[1], I.w = (int)r[2];
  I.xb = tables + r[3], I.xk = I.xb + 2 * ow;
  I.yb = tables + r[4], I.yk = I.yb + 2 * oh;
  I.kx = (int)r[5], I.ky = (int)r[6];
  I.ws_off = r[7];
  I.y0 = (int)r[8];
  I.rows = I.yb[2 * (oh - 1)] + I.yb[2 * (oh - 1) + 1] - I.y0;  // source rows y0 .. y0 + rows - 1 are read
  return I;
}

__device__ __forceinline__ int rs_clip8(int acc) { return min(max(acc >> RS_PRECISION_BITS, 0), 255); }

// grid (ceil(ow * c / 256), ceil(max_rows / RS_ROWS), n); a thread owns output (xx, ch) of RS_ROWS source rows
__global__ void __launch_bounds__(256) resample_x_kernel(const uint8_t* __restrict__ src,
                                                         const int64_t* __restrict__ recs,
                                                         const int32_t* __restrict__ tables, uint8_t* __restrict__ ws,
                                                         int c, int oh, int ow) {
  const RsImage I = rs_image(recs, tables, blockIdx.z, oh, ow);
  const int r0 = blockIdx.y * RS_ROWS;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (r0 >= I.rows || j >= ow * c) return;
  const int xx = j / c, ch = j - xx * c;
  const int xmin = I.xb[2 * xx], taps = I.xb[2 * xx + 1];
  const int32_t* k = I.xk + (int64_t)xx * I.kx;
  const int64_t pitch = (int64_t)I.w * c;
  const uint8_t* p[RS_ROWS];
  int acc[RS_ROWS];
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r) {
    // a row past the last one re-reads the last (inside the image); its sum is not stored
    p[r] = src + I.src_off + (int64_t)(I.y0 + min(r0 + r, I.rows - 1)) * pitch + (int64_t)xmin * c + ch;
    acc[r] = 1 << (RS_PRECISION_BITS - 1);
  }
  for (int t = 0; t < taps; ++t) {
    const int kt = k[t];
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) acc[r] += (int)p[r][t * c] * kt;
  }
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r)
    if (r0 + r < I.rows) ws[I.ws_off + (int64_t)(r0 + r) * ow * c + j] = (uint8_t)rs_clip8(acc[r]);
}

// grid (ceil(ow * c / 256), oh, n); a thread owns output (yy, xx, ch).  LUT: f32 NCHW through the table, threads
// ordered (ch, xx) so each plane's row is stored contiguously; else uint8 HWC, threads ordered (xx, ch).
template <bool LUT>
__global__ void __launch_bounds__(256) resample_y_kernel(const int64_t* __restrict__ recs,
                                                         const int32_t* __restrict__ tables,
                                                         const uint8_t* __restrict__ ws, void* __restrict__ out,
                                                         const float* __restrict__ lut, int c, int oh, int ow) {
  const int img = blockIdx.z, yy = blockIdx.y;
  const RsImage I = rs_image(recs, tables, img, oh, ow);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ow * c) return;
  int xx, ch;
  if (LUT)
    ch = j / ow, xx = j - ch * ow;
  else
    xx = j / c, ch = j - xx * c;
  const int ymin = I.yb[2 * yy], taps = I.yb[2 * yy + 1];
  const int32_t* k = I.yk + (int64_t)yy * I.ky;
  const int64_t pitch = (int64_t)ow * c;
  const uint8_t* p = ws + I.ws_off + (int64_t)(ymin - I.y0) * pitch + xx * c + ch;
  int acc = 1 << (RS_PRECISION_BITS - 1);
  for (int t = 0; t < taps; ++t) acc += (int)p[t * pitch] * k[t];
  const int v = rs_clip8(acc);
  if (LUT)
    static_cast<float*>(out)[(((int64_t)img * c + ch) * oh + yy) * ow + xx] = lut[ch * 256 + v];
  else
    static_cast<uint8_t*>(out)[((int64_t)img * oh + yy) * pitch + j] = (uint8_t)v;
}

// ---------------------------------------------------------------------------------------------- f32 -> uint8
__device__ __forceinline__ int image_u8(float v, int mode) {
#pragma clang fp contract(off)  // one rounding per written operation
  if (mode == IC2_U8_EVAL) return to_u8(v);
  if (mode == IC2_U8_SAVE_IMAGE) {
    const float t = (v + 1.f) / 2.f;
    float u = t * 255.f + 0.5f;
    u = fminf(fmaxf(u, 0.f), 255.f);  // fmaxf(NaN, 0) = 0
    return (int)u;
  }
  const float u = (v + 1.f) * 127.5f;
  if (!(u >= 0.f)) return 0;  // negative or NaN
  return u >= 256.f ? 255 : (int)u;
}

// grid (blocks per image * n); a thread owns four consecutive output bytes of one image (hwc = h * w * c of them)
__global__ void __launch_bounds__(256) image_to_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ y, int c,
                                                          int hw, int hwc, int bpi, int mode) {
  const int img = blockIdx.x / bpi;
  const int j0 = ((blockIdx.x - img * bpi) * 256 + threadIdx.x) * 4;
  if (j0 >= hwc) return;
  const float* xi = x + (int64_t)img * hwc;
  uint8_t* yi = y + (int64_t)img * hwc + j0;
  int v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = min(j0 + e, hwc - 1);
    const int pix = j / c, ch = j - pix * c;
    v[e] = image_u8(xi[(int64_t)ch * hw + pix], mode);
  }
  if (j0 + 3 < hwc && ((uintptr_t)yi & 3) == 0) {
    *reinterpret_cast<uint32_t*>(yi) =
        (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j0 + e < hwc) yi[e] = (uint8_t)v[e];
  }
}

}  // namespace ic2

using namespace ic2;

extern "C" int ic2_resample_ksize(int in, int out, int filter) {
#pragma clang fp contract(off)
  if (!rs_axis_ok(in, out, filter)) return 0;
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(rs_filter_support(filter) * fs) * 2 + 1;
}

extern "C" int ic2_resample_coeffs(int in, int out, int filter, int32_t* bounds, int32_t* kk) {
#pragma clang fp contract(off)  // one contracted multiply-add in `center` changes tables
  IC2_CHECK_ARG(bounds && kk, "resample_coeffs: null pointer (bounds and kk are required)");
  IC2_CHECK_ARG(filter >= IC2_RESAMPLE_BILINEAR && filter <= IC2_RESAMPLE_LANCZOS,
                "resample_coeffs: unknown filter %d (0 bilinear, 1 bicubic, 2 lanczos)", filter);
  IC2_CHECK_ARG(rs_axis_ok(in, out, filter), "resample_coeffs: in=%d out=%d must be within [1, %d]", in, out,
                RS_MAX_SIZE);
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = rs_filter_support(filter) * fs;
  const int ksize = (int)ceil(support) * 2 + 1;
  std::vector<double> w((size_t)ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      w[x] = rs_filter(filter, (x + xmin - center + 0.5) / fs);
      ww += w[x];
    }
    int32_t* k = kk + (int64_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      if (x >= xmax) {
        k[x] = 0;
        continue;
      }
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      k[x] = v < 0.0 ? (int)(v * (double)(1 << RS_PRECISION_BITS) - 0.5)
                     : (int)(v * (double)(1 << RS_PRECISION_BITS) + 0.5);
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return IC2_OK;
}

extern "C" int ic2_resample_u8(const uint8_t* src, const int64_t* recs, const int32_t* tables, int n, int c, int oh,
                               int ow, int max_rows, int64_t total_rows, uint8_t* ws, int64_t ws_bytes, void* out,
                               const float* lut, void* stream) {
  IC2_CHECK_ARG(src && recs && tables && ws && out,
                "resample_u8: null pointer (src, recs, tables, ws and out are required)");
  IC2_CHECK_ARG(n > 0 && n <= 65535, "resample_u8: n=%d must be within [1, 65535]", n);
  IC2_CHECK_ARG(c == 1 || c == 3, "resample_u8: c=%d must be 1 or 3", c);
  IC2_CHECK_ARG(oh > 0 && oh <= RS_MAX_SIZE && ow > 0 && ow <= RS_MAX_SIZE,
                "resample_u8: oh=%d ow=%d must be within [1, %d]", oh, ow, RS_MAX_SIZE);
  IC2_CHECK_ARG(max_rows > 0 && max_rows <= RS_MAX_SIZE && total_rows >= max_rows && total_rows <= (int64_t)n * max_rows,
                "resample_u8: max_rows=%d total_rows=%lld do not describe %d images of at most %d rows", max_rows,
                (long long)total_rows, n, RS_MAX_SIZE);
  IC2_CHECK_ARG(ws_bytes >= total_rows * ow * c,
                "resample_u8: workspace of %lld bytes, %lld rows of ow * c = %d bytes need %lld", (long long)ws_bytes,
                (long long)total_rows, ow * c, (long long)(total_rows * ow * c));
  hipStream_t s = as_stream(stream);
  const unsigned bx = (unsigned)ceil_div((int64_t)ow * c, 256);
  hipLaunchKernelGGL(resample_x_kernel, dim3(bx, (unsigned)ceil_div(max_rows, RS_ROWS), (unsigned)n), dim3(256), 0, s,
                     src, recs, tables, ws, c, oh, ow);
  if (lut)
    hipLaunchKernelGGL(resample_y_kernel<true>, dim3(bx, (unsigned)oh, (unsigned)n), dim3(256), 0, s, recs, tables, ws,
                       out, lut, c, oh, ow);
  else
    hipLaunchKernelGGL(resample_y_kernel<false>, dim3(bx, (unsigned)oh, (unsigned)n), dim3(256), 0, s, recs, tables,
                       ws, out, lut, c, oh, ow);
  IC2_CHECK_LAUNCH("resample_u8");
  return IC2_OK;
}

extern "C" int ic2_image_to_u8(const float* x, uint8_t* y, int n, int c, int h, int w, int mode, void* stream) {
  IC2_CHECK_ARG(x && y, "image_to_u8: null pointer (x and y are required)");
  IC2_CHECK_ARG(n > 0 && c > 0 && h > 0 && w > 0, "image_to_u8: n=%d c=%d h=%d w=%d must be positive", n, c, h, w);
  IC2_CHECK_ARG(mode >= IC2_U8_EVAL && mode <= IC2_U8_REFERENCE,
                "image_to_u8: unknown mode %d (0 eval, 1 save_image, 2 reference)", mode);
  const int64_t hwc = (int64_t)h * w * c;
  IC2_CHECK_ARG(hwc <= INT32_MAX - 4, "image_to_u8: c=%d h=%d w=%d is more than one image's int32 index holds", c, h,
                w);
  const int64_t bpi = ceil_div(ceil_div(hwc, 4), 256);
  IC2_CHECK_ARG(bpi * n <= INT32_MAX, "image_to_u8: n=%d c=%d h=%d w=%d is more blocks than one launch holds", n, c,
                h, w);
  hipLaunchKernelGGL(image_to_u8_kernel, dim3((unsigned)(bpi * n)), dim3(256), 0, as_stream(stream), x, y, c, h * w,
                     (int)hwc, (int)bpi, mode);
  IC2_CHECK_LAUNCH("image_to_u8");
  return IC2_OK;
}
