// Fused filtered leaky-ReLU on the matrix cores: the NHWC / NHWC16 synthesis path of
// SynthesisLayer.forward [SG3-public filtered_lrelu: bias_act -> upfirdn2d(fu, up) -> lrelu*gain, clamp
// -> upfirdn2d(fd, down)], called for every layer of G.synthesis (/root/reference/stylegan3_hvae_full.py:274,329).
//
// Two kernels: flrelu_mfma3_kernel (strip-streaming, f16 input) is the product kernel, every launch of the
// synthesis goes to it; flrelu_mfma_kernel (16x16 tiles) serves the C ABI's bf16 input only.
//
// Every separable FIR pass is a small banded matrix applied along one axis, and the FIR never mixes
// channels, so each pass is an MFMA with 16 channels on one side and 16 positions along the filtered
// axis on the other:
//   vertical up     V^T[c][ky] = X^T[c][jy] . Gu^T[jy][ky]      (A from LDS by transposed read)
//   horizontal up   U[kx][c]   = Gu[kx][jx] . V[jx][c]          (B from LDS by transposed read)
//   activation      lrelu(U) * gain, clamp  (on the accumulator, after its conversion to f16)
//   horizontal down D^T[c][ox] = act(U)^T[c][kx] . GdT[kx][ox]  (the accumulator IS the A operand)
//   vertical down   O^T[c][oy] = D^T[c][ky] . GdT[ky][oy]       (A from LDS by transposed read)
// The filter matrices are built once per workgroup into registers (f16 taps); 16x16x16 MFMAs for the
// up passes (a 16-output band spans <= 14 inputs), 16x16x32 where K can be filled (horizontal down).
// The up-sampled grid exists only 16 rows at a time in LDS; persistent workgroups loop over their work items.
#include "flrelu_mfma.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace ic2 {

template <int U>
struct FmGeom {
  static constexpr int TU = 6 * U, TD = 12;
  static constexpr int TO = 16;                        // output tile side
  static constexpr int RA = (TO - 1) * 2 + TD;         // 42 lrelu-grid rows / columns per tile
  static constexpr int NIN = (RA + TU - 2) / U + 1;    // 27 (up 2) / 17 (up 4) input rows / columns
  static constexpr int NB = (RA + 15) / 16;            // 3 grid blocks of 16
  // LDS images (dwords); pitches chosen for conflict-free transposed reads / b64 writes
  static constexpr int IN_PITCH = NIN * 8;             // [jy][x][16 ch]: NIN odd -> 8 rows hit 8 bank groups
  static constexpr int IN_DW = (NIN * NIN * 2 + 63) / 64 * 256;  // 16-B chunks, rounded up to whole KiB
  static constexpr int V_PITCH = NIN * 8 + 2;          // [ky][x][16 ch]: 16 rows of b64 writes hit 16 bank pairs
  static constexpr int V_DW = 16 * V_PITCH;
  static constexpr int D_XP = 10;                      // [ky][ox][16 ch], ox pitch 10 dwords
  static constexpr int D_PITCH = 16 * D_XP + 8;        // 168 = 40 mod 64: 8 rows hit 8 bank groups
  static constexpr int D_DW = 16 * D_PITCH;
  static constexpr int LDS_DW = IN_DW + V_DW + D_DW + FM_TAPS;
  static_assert(NIN % 2 == 1 && NIN >= 16, "input image width must be odd and cover a 16-wide window");
};

// first input sample feeding grid position i (polyphase), then clipped so a 16-wide window stays
// inside the NIN-sample image (taps outside the band are zero, so a window shifted back is exact)
template <int U, int DELTA, int NIN>
__device__ constexpr int fm_win(int i) {
  const int j = i < DELTA ? 0 : (i - DELTA + U - 1) / U;
  return j < NIN - 16 ? j : NIN - 16;
}

// bf16 pair -> f16 pair, saturated to the f16 range (a pre-activation beyond +-65504 ends up clamped
// by the activation anyway)
__device__ __forceinline__ uint32_t fm_bf2_to_h2(uint32_t v) {
  const float lo = __builtin_amdgcn_fmed3f(__uint_as_float(v << 16), -65504.f, 65504.f);
  const float hi = __builtin_amdgcn_fmed3f(__uint_as_float(v & 0xffff0000u), -65504.f, 65504.f);
  return fm_h2u(lo, hi);
}

// the output quad (bf16, or f16 saturated in the synthesis's f16 mode)
__device__ __forceinline__ uint2 fm_out4(bool f16, float a, float b, float c, float d) {
  if (f16) {
    const float lo = -65504.f, hi = 65504.f;
    return fm_pack4(__builtin_amdgcn_fmed3f(a, lo, hi), __builtin_amdgcn_fmed3f(b, lo, hi),
                    __builtin_amdgcn_fmed3f(c, lo, hi), __builtin_amdgcn_fmed3f(d, lo, hi));
  }
  return make_uint2((uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16), (uint32_t)f2bf(c) | ((uint32_t)f2bf(d) << 16));
}

// the same on an f16 pair, after the conversion the next MFMA needs anyway: 3 packed instructions per pair
// (slope*v, maximum3(v, slope*v, -lim) = lrelu clamped from below, min(., lim)).  f16 rounding happens
// before the activation instead of after it: for v >= 0 identical, for v < 0 slope*f16(v) vs f16(slope*v)
// differ by <= 1 ulp of f16 (the operand is f16 either way).
// Two pairs per asm block, interleaved (one block keeps the compiler from padding dependent inline-asm
// instructions with s_nop; plain VALU RAW dependences interlock in hardware).
__device__ __forceinline__ uint2 fm_act_h4(uint32_t h0, uint32_t h1, uint32_t slope2, uint32_t nlim2, uint32_t lim2) {
  uint32_t t0, t1;
  asm("v_pk_mul_f16 %2, %0, %4\n\t"
      "v_pk_mul_f16 %3, %1, %4\n\t"
      "v_pk_maximum3_f16 %0, %0, %2, %5\n\t"
      "v_pk_maximum3_f16 %1, %1, %3, %5\n\t"
      "v_pk_min_f16 %0, %0, %6\n\t"
      "v_pk_min_f16 %1, %1, %6"
      : "+v"(h0), "+v"(h1), "=&v"(t0), "=&v"(t1)
      : "v"(slope2), "v"(nlim2), "v"(lim2));
  return make_uint2(h0, h1);
}

// clamp-split activation for a finite clamp (CL kernels): the up pass produces u' = u / lim, and
//   lrelu(u) clamped to [-lim, lim] = lim * (clamp01(u') - clamp01(-slope * u'))
// (u >= 0: min(u, lim); u < 0: max(slope * u, -lim)), so after the f16 conversion each pair costs two packed
// instructions with the hardware [0, 1] clamp; the factor lim and the subtraction go into the down-pass
// matrices, whose K doubles (positive and negative parts), on the otherwise idle matrix pipe.
__device__ __forceinline__ void fm_act_split(uint32_t h0, uint32_t h1, uint32_t nslope2, uint2& pos, uint2& neg) {
  uint32_t p0, p1, n0, n1;
  asm("v_pk_max_f16 %0, %4, 0 clamp\n\t"
      "v_pk_max_f16 %1, %5, 0 clamp\n\t"
      "v_pk_mul_f16 %2, %4, %6 clamp\n\t"
      "v_pk_mul_f16 %3, %5, %6 clamp"
      : "=&v"(p0), "=&v"(p1), "=&v"(n0), "=&v"(n1)
      : "v"(h0), "v"(h1), "v"(nslope2));
  pos = make_uint2(p0, p1);
  neg = make_uint2(n0, n1);
}

// ------------------------------------------------------------------------------------------------
// Tile kernel: the bf16-input instance of the C ABI (ic2_flrelu_nhwc / ic2_flrelu_nhwc16 with IC2_BF16 input and
// NHWC output).  The synthesis does not call it: its conv output is f16 and goes to the strip kernel below.
// A tile = one sample x one 16x16 output tile x 16 channels; 4 waves split columns / rows / output columns of
// each 16-row grid block; separate V and D images in LDS.
template <int U, int DELTA>
__global__ void __launch_bounds__(256) flrelu_mfma_kernel(FlrArgs a, int ntiles) {
  constexpr int NW = 4, NT = 64 * NW, RR = 16 / NW;  // waves, threads; grid rows (and output columns) per wave per block
  using G = FmGeom<U>;
  constexpr int NIN = G::NIN, NCH = NIN * NIN * 2;  // input pixels x 16-B halves
  __shared__ __attribute__((aligned(16))) uint32_t lds[G::LDS_DW];
  uint32_t* const in_img = lds;
  uint32_t* const v_img = lds + G::IN_DW;
  uint32_t* const d_img = v_img + G::V_DW;
  float* const taps = reinterpret_cast<float*>(d_img + G::D_DW);  // FM_TAPS floats, layout below

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int tq = li >> 2, tp = li & 3;  // this lane's (row, 4-column group) in a transposed read

  // tap tables with zero guard bands, so every per-lane filter-matrix entry below is a branch-free read
  // (tap ranges: up [-43, 63], down [-30, 47]): gu at [48, 72) of [0, 116), gd at [148, 160) of [116, 196),
  // gdg (gain folded) at [228, 240) of [196, 276)
  for (int i = tid; i < FM_TAPS; i += NT) {
    float v = 0.f;
    if (i >= 48 && i < 72) v = a.gu[i - 48];
    else if (i >= 148 && i < 160) v = a.gd[i - 148];
    else if (i >= 228 && i < 240) v = a.gdg[i - 228];
    taps[i] = v;
  }

  // persistent: this workgroup runs tiles slot, slot + gridDim.x, ...  Logical tiles run channel block
  // fastest and consecutive slots share an XCD, so the channel blocks of one tile (16 channels = 32 B of
  // each 128-B line of the input) are fetched once into that XCD's L2.
  const int slot = fm_xcd_remap(blockIdx.x, gridDim.x);
  const uint16_t* xin = reinterpret_cast<const uint16_t*>(a.x);
  auto tile_geom = [&](int t, int& n, int& oy0, int& ox0, int& c0) {
    const int cb = t % a.cblocks;
    t /= a.cblocks;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    const int ty = t % a.tiles_y;
    n = t / a.tiles_y;
    oy0 = ty * 16;
    ox0 = tx * 16;
    c0 = cb * 16;
  };
  // input tile -> in_img[jy][x][16 ch] as f16 (zeros outside the image): chunk e = (pixel, 16-B half), one
  // 16-B load per chunk, converted on the way to LDS
  auto chunk_src = [&](int e, int n, int sy0, int sx0, int c0) -> const void* {
    const int pix = e >> 1, half = e & 1;
    const int jy = pix / NIN, x = pix - jy * NIN;
    const int iy = sy0 + jy, ix = sx0 + x;
    const bool ok = e < NCH && (unsigned)iy < (unsigned)a.in_h && (unsigned)ix < (unsigned)a.in_w;
    const uint16_t* src = xin + n * a.xsn + (c0 >> 4) * a.xcb + iy * a.xsy + ix * a.xsx + half * 8;
    return ok ? (const void*)src : zero_line();
  };
  auto load_tile = [&](int t) {
    int n, oy0, ox0, c0;
    tile_geom(t, n, oy0, ox0, c0);
    const int sy0 = (oy0 * 2 - a.py0 + DELTA) / U, sx0 = (ox0 * 2 - a.px0 + DELTA) / U;
    constexpr int PER = (NCH + NT - 1) / NT;
    uint4 v[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r)  // every load in flight before the first conversion
      v[r] = *reinterpret_cast<const uint4*>(chunk_src(tid + NT * r, n, sy0, sx0, c0));
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int e = tid + NT * r;
      if (e < NCH)
        *reinterpret_cast<uint4*>(in_img + e * 4) =
            make_uint4(fm_bf2_to_h2(v[r].x), fm_bf2_to_h2(v[r].y), fm_bf2_to_h2(v[r].z), fm_bf2_to_h2(v[r].w));
    }
  };
  __syncthreads();  // taps

  // ---- filter matrices (f16: 11-bit taps; bf16 taps cost 5e-3 mean relative error on the critically
  // sampled layers) in registers, once per workgroup
  // gmat[t]: Gu[16t + li][win(16t) + 4g + j]  (B of the vertical pass, A of the horizontal pass)
  fm_h4 gmat[G::NB];
#pragma unroll
  for (int t = 0; t < G::NB; ++t) {
    const int w0 = fm_win<U, DELTA, NIN>(16 * t);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tap = U * (w0 + 4 * g + j) + DELTA - (16 * t + li);
      v[j] = taps[48 + tap];
    }
    gmat[t] = fm_h4_of(fm_pack4(v[0], v[1], v[2], v[3]));
  }
  // horizontal down (gain folded): GdT[kx][ox = li]; x32 operands over kx blocks (0,1) and (2, zero)
  fm_h8 gdh01, gdh2;
  {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kx = (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
      v[j] = taps[228 + kx - 2 * li];
    }
    gdh01 = fm_h8_of(fm_pack4(v[0], v[1], v[2], v[3]), fm_pack4(v[4], v[5], v[6], v[7]));
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = taps[228 + 32 + 4 * g + j - 2 * li];
    gdh2 = fm_h8_of(fm_pack4(v[0], v[1], v[2], v[3]), make_uint2(0u, 0u));
  }
  // vertical down: GdT[ky = 16b + 4g + j][oy = li]
  fm_h4 gdv[G::NB];
#pragma unroll
  for (int b = 0; b < G::NB; ++b) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = taps[148 + 16 * b + 4 * g + j - 2 * li];
    gdv[b] = fm_h4_of(fm_pack4(v[0], v[1], v[2], v[3]));
  }
  const float slope = a.slope, lim = a.lim;
  const uint32_t slope2 = fm_h2u(slope, slope), lim2 = fm_h2u(lim, lim), nlim2 = fm_h2u(-lim, -lim);
  bf16_t* yout = reinterpret_cast<bf16_t*>(a.y);

  for (int t = slot; t < ntiles; t += gridDim.x) {
    int n, oy0, ox0, c0;
    tile_geom(t, n, oy0, ox0, c0);
    load_tile(t);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's loads (and last tile's stores)
    __syncthreads();                                   // everyone's; and the previous tile fully consumed

    fm_f4 acc[RR];
#pragma unroll
    for (int i = 0; i < RR; ++i) acc[i] = fm_f4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int b = 0; b < G::NB; ++b) {
      // ---- vertical up: V^T[c][ky] for the 16 grid rows of block b, every input column.  Fixed trip
      // count; the tail columns past NIN repeat column NIN-1 (identical bytes to the same place).  Issued
      // as groups (every column's LDS read, then every MFMA, then every store) with scheduling barriers
      // between them, so the columns' LDS and MFMA latencies overlap instead of forming one serial chain
      {
        constexpr int NC = (NIN + NW - 1) / NW;
        const int w0 = fm_win<U, DELTA, NIN>(16 * b);
        fm_s4 xa[NC];
        fm_f4 vt[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
          const int x = min(wave + NW * i, NIN - 1);
          xa[i] = fm_tr_read(in_img + (w0 + 4 * g + tq) * G::IN_PITCH + x * 8 + 2 * tp);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NC; ++i)
          vt[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(fm_h4, xa[i]), gmat[b],
                                                        fm_f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
          const int x = min(wave + NW * i, NIN - 1);
          *reinterpret_cast<uint2*>(v_img + li * G::V_PITCH + x * 8 + 2 * g) =
              fm_pack4(vt[i][0], vt[i][1], vt[i][2], vt[i][3]);
        }
      }
      __syncthreads();
      // ---- horizontal: up, activation, down, for this wave's 4 grid rows of the block (the rows past RA in
      // the last block too: finite, and weighted by zero in the vertical down; no branch, so the rows'
      // MFMA chains interleave)
      // grouped like the vertical pass: all 12 LDS reads, all 12 up MFMAs, the activations, the 8 down
      // MFMAs, the stores
      fm_s4 vb[RR][G::NB];
#pragma unroll
      for (int rr = 0; rr < RR; ++rr)
#pragma unroll
        for (int tt = 0; tt < G::NB; ++tt) {
          const int w0 = fm_win<U, DELTA, NIN>(16 * tt);
          vb[rr][tt] = fm_tr_read(v_img + (wave + NW * rr) * G::V_PITCH + (w0 + 4 * g + tq) * 8 + 2 * tp);
        }
      __builtin_amdgcn_sched_barrier(0);
      fm_f4 u[RR][G::NB];
#pragma unroll
      for (int rr = 0; rr < RR; ++rr)
#pragma unroll
        for (int tt = 0; tt < G::NB; ++tt)
          u[rr][tt] = __builtin_amdgcn_mfma_f32_16x16x16f16(gmat[tt], __builtin_bit_cast(fm_h4, vb[rr][tt]),
                                                            fm_f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      fm_h4 au[RR][G::NB];
#pragma unroll
      for (int rr = 0; rr < RR; ++rr)
#pragma unroll
        for (int tt = 0; tt < G::NB; ++tt)
          au[rr][tt] = fm_h4_of(fm_act_h4(fm_h2u(u[rr][tt][0], u[rr][tt][1]), fm_h2u(u[rr][tt][2], u[rr][tt][3]),
                                          slope2, nlim2, lim2));
      __builtin_amdgcn_sched_barrier(0);
      fm_f4 d[RR];
#pragma unroll
      for (int rr = 0; rr < RR; ++rr) {
        const uint2 a0 = __builtin_bit_cast(uint2, au[rr][0]), a1 = __builtin_bit_cast(uint2, au[rr][1]);
        d[rr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fm_h8_of(a0, a1), gdh01, fm_f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
      // block 2 as a second 16x16x32 with a zero upper half: a 16x16x16 accumulating onto the 16x16x32's
      // result one instruction later reads stale rows 0-1 of the accumulator (mixed-shape srcC hazard)
#pragma unroll
      for (int rr = 0; rr < RR; ++rr) {
        const uint2 a2 = __builtin_bit_cast(uint2, au[rr][2]);
        d[rr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fm_h8_of(a2, make_uint2(0u, 0u)), gdh2, d[rr], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int rr = 0; rr < RR; ++rr) {
        *reinterpret_cast<uint2*>(d_img + (wave + NW * rr) * G::D_PITCH + li * G::D_XP + 2 * g) =
            fm_pack4(d[rr][0], d[rr][1], d[rr][2], d[rr][3]);
      }
      __syncthreads();
      // ---- vertical down: accumulate block b's 16 grid rows into this wave's 4 output columns
      fm_s4 da[RR];
#pragma unroll
      for (int i = 0; i < RR; ++i)
        da[i] = fm_tr_read(d_img + (4 * g + tq) * G::D_PITCH + (wave + NW * i) * G::D_XP + 2 * tp);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < RR; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(fm_h4, da[i]), gdv[b], acc[i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- store: lane (g, oy = li) holds channels c0 + 4g .. +3 of output pixel (oy, ox)
    float ps[4] = {1.f, 1.f, 1.f, 1.f};
    if (a.post_scale) {
      const float4 p = *reinterpret_cast<const float4*>(a.post_scale + (int64_t)n * a.c_p + c0 + 4 * g);
      ps[0] = p.x; ps[1] = p.y; ps[2] = p.z; ps[3] = p.w;
    }
    const int gy = oy0 + li;
#pragma unroll
    for (int i = 0; i < RR; ++i) {
      const int gx = ox0 + wave + NW * i;
      if (gy < a.out_h && gx < a.out_w) {
        const uint2 v = fm_out4(a.out_f16, acc[i][0] * ps[0], acc[i][1] * ps[1], acc[i][2] * ps[2], acc[i][3] * ps[3]);
        *reinterpret_cast<uint2*>(yout + (((int64_t)n * a.out_h + gy) * a.out_w + gx) * a.c_p + c0 + 4 * g) = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Strip-streaming kernel (f16 input: the synthesis path).
// A work item is a strip: one sample x 32 output columns x 16 channels x a
// run of consecutive 16-row tiles, walked top to bottom.  Tile t needs lrelu-grid rows 32t .. 32t+41, i.e. grid
// blocks 2t, 2t+1, 2t+2 of 16 rows, and block 2t+2 is block 0 of tile t+1: the strip computes every grid block
// once (2 per tile instead of 3) and carries that shared block's vertical-down contribution to the next tile in
// registers (acc_b).  Its input rows live in an LDS ring of U+1 groups of 16/U rows: block k reads rows
// 16k/U .. 16k/U+15 (strip-relative; with DELTA = py0 mod U this window covers every tap of the block's rows for
// every k, so one vertical-up matrix serves all blocks), and after block k's vertical up the group it no longer
// needs is refilled with the rows block k+2 will need: 16/U new input rows per block (16 / 8 per 16 output rows,
// up 2 / 4) instead of the tile kernel's 27 / 17.
// Horizontally a strip is 32 output columns wide on 8 waves: the 12-tap down filter needs 2 * 31 + 12 = 74 grid
// columns (5 blocks of 16), i.e. 7.5 lrelu-grid points per output against the 16-column tile's 9, and each phase's
// barrier is amortised over twice the outputs.  The horizontal down pass of output block ob reads grid blocks
// 2 ob .. 2 ob + 2 with the block-0 matrices (the band is translation invariant).  The tap table aliases the D image
// (it is only read before the first strip), which keeps 2 workgroups = 16 waves per CU.
template <int U>
struct FmGeom3 {
  static constexpr int TU = 6 * U, TD = 12, TOX = 32;
  static constexpr int RAX = (TOX - 1) * 2 + TD;   // 74 grid columns
  static constexpr int NINX = (RAX + TU - 2) / U + 1;  // 43 (up 2) / 25 (up 4) input columns
  static constexpr int NBX = (RAX + 15) / 16;      // 5 grid column blocks
  static constexpr int NOB = TOX / 16;             // output column blocks
  static constexpr int V_PITCH = NINX * 8 + 2;     // [ky][x][16 ch]: 16 rows of b64 writes hit 16 bank pairs
  static constexpr int V_DW = 16 * V_PITCH;
  static constexpr int D_XP = 10;                  // [ky][ox][16 ch], ox pitch 10 dwords
  static constexpr int D_PITCH = TOX * D_XP + 8;
  static constexpr int D_DW = 16 * D_PITCH;
  static constexpr int DT_DW = D_DW > FM_TAPS_CL ? D_DW : FM_TAPS_CL;  // D image, aliased by the tap table
  static_assert(NBX == 2 * NOB + 1, "horizontal down: output block ob reads grid blocks 2ob .. 2ob+2");
  static constexpr int S = 16 / U;             // input rows per grid block (8 / 4)
  static constexpr int NG = U + 1;             // ring groups of S rows
  static constexpr int IN_PITCH = NINX * 8;    // dwords per input row [x][16 ch]; NINX odd
  static constexpr int GCH = S * NINX * 2;     // 16-B chunks per group
  static constexpr int NGI = (GCH + 63) / 64;  // 1-KiB DMA instructions per group
  static constexpr int GRP_DW = NGI * 256;
  static constexpr int RING_DW = NG * GRP_DW;
  static constexpr int LDS_DW = RING_DW + V_DW + DT_DW + 16;  // + the strip's 16 post-scale floats
  static_assert(U * S == 16 && NINX % 2 == 1, "geometry");
  // the surplus columns' reads (x < NW * ceil(NINX / NW)) of the last row of the last group stay in the ring
  static_assert((NG - 1) * GRP_DW + (S - 1) * IN_PITCH + 8 * 8 * ((NINX + 7) / 8) <= RING_DW, "ring bounds");
};

// 4 x 4 transpose of 8-byte elements over a lane quad: on return lane p of a quad holds in v[i] what lane i held in
// v[p].  Two butterfly stages (quad_perm xor 1, xor 2); in each, a lane sends the element its partner keeps the slot
// of and receives into the slot it gives up.
__device__ __forceinline__ void fm_quad_transpose(uint2 (&v)[4], int p) {
  const bool b0 = (p & 1) != 0, b1 = (p & 2) != 0;
  auto swap = [](uint32_t& lo, uint32_t& hi, bool up, auto ctrl) {
    constexpr int CTRL = decltype(ctrl)::value;
    const uint32_t send = up ? lo : hi;
    const uint32_t recv = (uint32_t)__builtin_amdgcn_mov_dpp((int)send, CTRL, 0xf, 0xf, true);
    lo = up ? recv : lo;
    hi = up ? hi : recv;
  };
  using X1 = std::integral_constant<int, 0xB1>;  // quad_perm [1, 0, 3, 2]
  using X2 = std::integral_constant<int, 0x4E>;  // quad_perm [2, 3, 0, 1]
#pragma unroll
  for (int i = 0; i < 4; i += 2) {
    swap(v[i].x, v[i + 1].x, b0, X1{});
    swap(v[i].y, v[i + 1].y, b0, X1{});
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    swap(v[i].x, v[i + 2].x, b1, X2{});
    swap(v[i].y, v[i + 2].y, b1, X2{});
  }
}

// BLK: channel-blocked NHWC16 output [n][c_p/16][out_h][out_w][16] (the hand-off to a conv that reads it blocked).  A
// wave then owns the 4 adjacent output columns 4 wave .. 4 wave + 3 (instead of wave + NW i) and transposes the 4
// columns x 4 rows held by each lane quad before the store, so the 16 lanes (4 columns x 4 channel quads) of one row
// fill one 128-B line; stored 16 B per lane, every store instruction of an interior tile writes 8 whole lines.
template <int U, int DELTA, int NW, bool CL, bool BLK>
__global__ void __launch_bounds__(64 * NW, 32 / NW) flrelu_mfma3_kernel(FlrArgs a, int nitems, int nseg, int seg_len) {
  using G = FmGeom3<U>;
  constexpr int TOX = G::TOX, NT = 64 * NW, RR = 16 / NW, OCW = TOX / NW;
  // output store instructions per wave per tile, exact and known here: the vmcnt waits below count them
  constexpr int NST = BLK ? OCW / 2 : OCW;
  constexpr int NINX = G::NINX, NBX = G::NBX, NOB = G::NOB, S = G::S, NG = G::NG;
  __shared__ __attribute__((aligned(16))) uint32_t lds[G::LDS_DW];
  uint32_t* const ring = lds;
  uint32_t* const v_img = lds + G::RING_DW;
  uint32_t* const d_img = v_img + G::V_DW;
  float* const taps = reinterpret_cast<float*>(d_img);  // read only before the first strip
  uint32_t* const ps_lds = d_img + G::DT_DW;             // the strip's post-scale row (DMA'd with its first rows)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int tq = li >> 2, tp = li & 3;
  // this lane's row in a vertical-up window, as (ring group offset, row in group)
  const int qoff = (4 * g + tq) / S, roff = (4 * g + tq) % S;

  for (int i = tid; i < FM_TAPS_CL; i += NT) {
    float v = 0.f;
    if (i >= 48 && i < 72) v = a.gu[i - 48];
    else if (i >= 148 && i < 160) v = a.gd[i - 148];
    else if (i >= 228 && i < 240) v = a.gdg[i - 228];
    else if (i >= 328 && i < 352) v = a.guh[i - 328];
    else if (i >= 428 && i < 440) v = a.gdgl[i - 428];
    taps[i] = v;
  }

  // work item w = ((n * tiles_x + tx) * nseg + seg) * cblocks + cb: the channel blocks of one strip run on
  // consecutive slots of one XCD, so they walk down together and their output stores (32 B of each pixel's
  // row each) meet in its L2
  const int slot = fm_xcd_remap(blockIdx.x, gridDim.x);
  const uint16_t* xin = reinterpret_cast<const uint16_t*>(a.x);
  auto item_geom = [&](int w, int& n, int& ox0, int& c0, int& t0, int& nt) {
    const int cb = w % a.cblocks;
    w /= a.cblocks;
    const int seg = w % nseg;
    w /= nseg;
    const int tx = w % a.tiles_x;
    n = w / a.tiles_x;
    ox0 = tx * TOX;
    c0 = cb * 16;
    t0 = seg * seg_len;
    nt = min(seg_len, a.tiles_y - t0);
  };
  const int xsy = (int)a.xsy, xsx = (int)a.xsx;  // < 2^31: checked by the launcher (per-sample image < 2 GiB)
  // group q (strip-relative input rows qS .. qS+S-1 of the item's first tile) -> ring slot q mod NG.  Which
  // (row, column, half) a lane moves is recomputed per DMA from an opaque copy of the lane id: hoisted out of the
  // item loop as loop invariants, these per-lane values pushed the kernel past 128 VGPRs into scratch
  // this wave's DMA instructions per ring group (wave-uniform; at most 2: the wait counts above)
  const int my_dma = wave < G::NGI ? (G::NGI - 1 - wave) / NW + 1 : 0;
  static_assert((G::NGI + NW - 1) / NW <= 2, "ring group DMA per wave");
  auto load_group = [&](int n, int iy0, int sx0, int c0, int q) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(xin + n * a.xsn + (c0 >> 4) * a.xcb), 0, FM_OOB, 0x00020000);
    uint32_t* const dst = ring + (q % NG) * G::GRP_DW;
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int i = 0; i < (G::NGI + NW - 1) / NW; ++i) {
      const int k = wave + NW * i;
      if (k < G::NGI) {
        const int e = k * 64 + ln;
        const int pix = e >> 1;
        const int row = pix / NINX, x = pix - row * NINX;
        const int iy = iy0 + q * S + row, ix = sx0 + x;
        const bool ok = e < G::GCH && (unsigned)iy < (unsigned)a.in_h && (unsigned)ix < (unsigned)a.in_w;
        const uint32_t off = ok ? (uint32_t)((iy * xsy + ix * xsx + (e & 1) * 8) * 2) : FM_OOB;
        fm_dma16(rs, off, dst + k * 256);
      }
    }
  };
  // an item's first U+1 groups and its post-scale row (every slot of the ring: issued only once the previous
  // item's last vertical up is done)
  auto load_item = [&](int w) __attribute__((always_inline)) {
    int n, ox0, c0, t0, nt;
    item_geom(w, n, ox0, c0, t0, nt);
    const int iy0 = (32 * t0 + DELTA - a.py0) / U, sx0 = (ox0 * 2 - a.px0 + DELTA) / U;
#pragma unroll
    for (int q = 0; q < NG; ++q) load_group(n, iy0, sx0, c0, q);
    if (a.post_scale != nullptr && wave == NW - 1 && lane < 4) {  // 64 B: post_scale[n][c0 .. c0 + 16)
      const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(a.post_scale + (int64_t)n * a.c_p + c0), 0, 64, 0x00020000);
      fm_dma16(prs, lane * 16, ps_lds);
    }
  };
  if (slot < nitems) load_item(slot);
  __syncthreads();  // taps

  // filter matrices.  Vertical up: grid row 16k + li of block k from input row kS + 4g + j, tap U(4g + j) +
  // DELTA - li (the same for every block)
  fm_h4 gmy, gmx[NBX];
  {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = taps[48 + U * (4 * g + j) + DELTA - li];
    gmy = fm_h4_of(fm_pack4(v[0], v[1], v[2], v[3]));
  }
#pragma unroll
  for (int t = 0; t < NBX; ++t) {
    const int w0 = fm_win<U, DELTA, NINX>(16 * t);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = taps[(CL ? 328 : 48) + U * (w0 + 4 * g + j) + DELTA - (16 * t + li)];
    gmx[t] = fm_h4_of(fm_pack4(v[0], v[1], v[2], v[3]));
  }
  fm_h8 gdh01, gdh2, gdq[3];
  {
    auto tap = [&](int blk, int j) { return taps[(CL ? 428 : 228) + 16 * blk + 4 * g + j - 2 * li]; };
    float v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = tap(0, j);
      v[4 + j] = tap(1, j);
    }
    gdh01 = fm_h8_of(fm_pack4(v[0], v[1], v[2], v[3]), fm_pack4(v[4], v[5], v[6], v[7]));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = tap(2, j);
      v[4 + j] = 0.f;
    }
    gdh2 = fm_h8_of(fm_pack4(v[0], v[1], v[2], v[3]), fm_pack4(v[4], v[5], v[6], v[7]));
#pragma unroll
    for (int bi = 0; bi < 3; ++bi) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = tap(bi, j);
        v[4 + j] = -tap(bi, j);
      }
      gdq[bi] = fm_h8_of(fm_pack4(v[0], v[1], v[2], v[3]), fm_pack4(v[4], v[5], v[6], v[7]));
    }
  }
  fm_h4 gdv[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = taps[148 + 16 * b + 4 * g + j - 2 * li];
    gdv[b] = fm_h4_of(fm_pack4(v[0], v[1], v[2], v[3]));
  }
  const float slope = a.slope, lim = CL ? 1.f : a.lim;
  const uint32_t slope2 = fm_h2u(slope, slope), lim2 = fm_h2u(lim, lim), nlim2 = fm_h2u(-lim, -lim);
  const uint32_t nslope2 = fm_h2u(-slope, -slope);
  bf16_t* yout = reinterpret_cast<bf16_t*>(a.y);
  __syncthreads();  // every wave's tap reads are done before the first D store overwrites the table

  bool first = true;
  for (int w = slot; w < nitems; w += gridDim.x) {
    int n, ox0, c0, t0, nt;
    item_geom(w, n, ox0, c0, t0, nt);
    const int iy0 = (32 * t0 + DELTA - a.py0) / U, sx0 = (ox0 * 2 - a.px0 + DELTA) / U;
    const bool has_next = w + (int)gridDim.x < nitems;
    // this wave's DMA of the item's first rows; the previous item's last NST output stores (issued after that
    // DMA, always exactly NST) stay in flight
    if (first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST) : "memory");
    first = false;
    __syncthreads();
    float4 psv = make_float4(1.f, 1.f, 1.f, 1.f);
    if (a.post_scale) psv = *reinterpret_cast<const float4*>(ps_lds + 4 * g);
    const float ps[4] = {psv.x, psv.y, psv.z, psv.w};
    // the sample's image, at this item's channels: 16 of every pixel's c_p (NHWC) or its own plane (BLK)
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(yout + (int64_t)n * a.out_h * a.out_w * a.c_p + (BLK ? (int64_t)c0 * a.out_h * a.out_w : (int64_t)c0)), 0,
        FM_OOB, 0x00020000);
    // Output row r of a tile reads grid rows 2r .. 2r + 11 of it, so the tile's second block (rows 32 .. 47) feeds rows
    // r >= 11 only: when the image's last tile has at most 11 live rows (every SG3 height but 256 leaves 4), the item
    // that ends with it stops one block early (uniform per item).  Every wait, DMA and hand-over below is keyed on kend.
    const bool tail_skip = t0 + nt == a.tiles_y && a.out_h - 16 * (a.tiles_y - 1) <= 11;
    const int kend = 2 * nt - (tail_skip ? 1 : 0);  // blocks 0 .. kend

    fm_f4 acc_a[OCW], acc_b[OCW];
    // store tile t0 + tt from acc_a: lane (g, oy = li) holds channels c0 + 4g .. +3 of output pixel (oy, ox); exactly
    // NST buffer stores per wave (out-of-range pixels at the dropped offset FM_OOB)
    auto store_tile = [&](int tt) __attribute__((always_inline)) {
      if constexpr (BLK) {
        // lane (g, li = 4 tq + tp) holds row li of columns 4 wave + i; after the quad transpose it holds column
        // 4 wave + tp of rows 4 tq + i: store i covers rows i, 4 + i, 8 + i, 12 + i, each one 128-B line of 4 pixels x
        // 32 B.  Exactly NST stores per wave (the vmcnt counts below)
        static_assert(OCW == 4, "quad transpose: 4 columns per wave");
        uint2 v[OCW];
#pragma unroll
        for (int i = 0; i < OCW; ++i)
          v[i] = fm_out4(a.out_f16, acc_a[i][0] * ps[0], acc_a[i][1] * ps[1], acc_a[i][2] * ps[2], acc_a[i][3] * ps[3]);
        fm_quad_transpose(v, tp);
        const int gy0 = 16 * (t0 + tt) + 4 * tq, gx = ox0 + 4 * wave + tp;
        // 16 B per lane: stores 2 h and 2 h + 1 trade halves across 16-lane rows (v_permlane16_swap: the odd rows of
        // its first operand with the even rows of its second), so the lanes of an even channel quad g hold channels
        // 4 g .. 4 g + 7 of store 2 h's pixel and those of an odd g channels 4 g - 4 .. 4 g + 3 of store 2 h + 1's:
        // one instruction writes 8 whole lines, NST = 2 instructions per wave per tile
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const auto x = __builtin_amdgcn_permlane16_swap(v[2 * h].x, v[2 * h + 1].x, false, false);
          const auto y = __builtin_amdgcn_permlane16_swap(v[2 * h].y, v[2 * h + 1].y, false, false);
          const int gy = gy0 + 2 * h + (g & 1);
          const uint32_t off =
              (gy < a.out_h && gx < a.out_w) ? (uint32_t)((gy * a.out_w + gx) * 32 + 16 * (g >> 1)) : FM_OOB;
          const v4u32_t q = {x[0], y[0], x[1], y[1]};
          __builtin_amdgcn_raw_buffer_store_b128(q, ors, off, 0, 0);
        }
        return;
      }
      const int gy = 16 * (t0 + tt) + li;
#pragma unroll
      for (int i = 0; i < OCW; ++i) {
        const int gx = ox0 + wave + NW * i;
        const uint32_t off =
            (gy < a.out_h && gx < a.out_w) ? (uint32_t)(((gy * a.out_w + gx) * a.c_p + 4 * g) * 2) : FM_OOB;
        const uint2 v = fm_out4(a.out_f16, acc_a[i][0] * ps[0], acc_a[i][1] * ps[1], acc_a[i][2] * ps[2], acc_a[i][3] * ps[3]);
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u32_t, v), ors, off, 0, 0);
      }
    };
    // grid block k of the item: vertical up (ring -> V), horizontal up / activation / down (V -> D), vertical down
    // (D -> acc).  MODE 0: block 0, starts acc_b; 1: odd block, acc_a = acc_b + its share; 2: even block >= 2,
    // finishes acc_a and starts acc_b for the next tile.  A finished tile is stored at the end of its even block (the
    // image's last tile after its odd block, under tail_skip).
    // END: the block may be the item's last (k == kend): an even block, or the odd block that ends a tail_skip item
    auto block = [&](int k, auto mode_c, auto end_c) __attribute__((always_inline)) {
      constexpr int MODE = decltype(mode_c)::value;
      constexpr bool END = decltype(end_c)::value;
      {  // vertical up
        constexpr int NC = (NINX + NW - 1) / NW;
        // column x = wave + NW i: one per-lane base per block and immediate offsets.  Columns past NINX - 1 (the
        // last round's surplus waves) read in-bounds bytes of the ring and are not stored
        const int q = k + qoff;
        const uint32_t* rowp = ring + (q % NG) * G::GRP_DW + roff * G::IN_PITCH + 2 * tp + wave * 8;
        fm_s4 xa[NC];
        fm_f4 vt[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) xa[i] = fm_tr_read(rowp + i * NW * 8);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NC; ++i)
          vt[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(fm_h4, xa[i]), gmy,
                                                        fm_f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        uint32_t* const vp = v_img + li * G::V_PITCH + 2 * g + wave * 8;
#pragma unroll
        for (int i = 0; i < NC; ++i)
          if (i < NC - 1 || wave + NW * i < NINX)
            *reinterpret_cast<uint2*>(vp + i * NW * 8) = fm_pack4(vt[i][0], vt[i][1], vt[i][2], vt[i][3]);
      }
      __syncthreads();  // V complete; the ring group k is dead; v-down k-1 done
      // the item's last block: every ring group is dead -> the next item's first rows
      if (END && k == kend && has_next) load_item(w + gridDim.x);
      // the rows block k+2 needs go out now, into the slot of group k (every wave's vertical up of block k is done):
      // they land behind this block's horizontal pass and vertical down and the next block's vertical up
      const bool dma = k + 2 <= kend;
      if (dma) load_group(n, iy0, sx0, c0, k + U + 1);
#pragma unroll
      for (int rr = 0; rr < RR; ++rr) {
        const int row = wave + NW * rr;
        fm_s4 vb[NBX];
#pragma unroll
        for (int tt = 0; tt < NBX; ++tt) {
          const int w0 = fm_win<U, DELTA, NINX>(16 * tt);
          vb[tt] = fm_tr_read(v_img + row * G::V_PITCH + (w0 + 4 * g + tq) * 8 + 2 * tp);
        }
        __builtin_amdgcn_sched_barrier(0);
        fm_f4 u[NBX];
#pragma unroll
        for (int tt = 0; tt < NBX; ++tt)
          u[tt] = __builtin_amdgcn_mfma_f32_16x16x16f16(gmx[tt], __builtin_bit_cast(fm_h4, vb[tt]),
                                                        fm_f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        fm_f4 d[NOB];
        if constexpr (CL) {
          fm_h8 qv[NBX];
#pragma unroll
          for (int tt = 0; tt < NBX; ++tt) {
            uint2 p, m;
            fm_act_split(fm_h2u(u[tt][0], u[tt][1]), fm_h2u(u[tt][2], u[tt][3]), nslope2, p, m);
            qv[tt] = fm_h8_of(p, m);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int bi = 0; bi < 3; ++bi)
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob)
              d[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qv[2 * ob + bi], gdq[bi],
                                                             bi == 0 ? fm_f4{0.f, 0.f, 0.f, 0.f} : d[ob], 0, 0, 0);
        } else {
          uint2 au[NBX];
#pragma unroll
          for (int tt = 0; tt < NBX; ++tt)
            au[tt] = fm_act_h4(fm_h2u(u[tt][0], u[tt][1]), fm_h2u(u[tt][2], u[tt][3]), slope2, nlim2, lim2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ob = 0; ob < NOB; ++ob)
            d[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fm_h8_of(au[2 * ob], au[2 * ob + 1]), gdh01,
                                                           fm_f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
          for (int ob = 0; ob < NOB; ++ob)
            d[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fm_h8_of(au[2 * ob + 2], make_uint2(0u, 0u)), gdh2, d[ob],
                                                           0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob)
          *reinterpret_cast<uint2*>(d_img + row * G::D_PITCH + (16 * ob + li) * G::D_XP + 2 * g) =
              fm_pack4(d[ob][0], d[ob][1], d[ob][2], d[ob][3]);
      }
      if (k >= 1 && k < kend) {
        // block k-1's ring DMA must have landed (block k+1 reads it); younger, and left in flight: the stores of the
        // tile finished at the end of block k-1 (odd k >= 3: exactly NST) and this block's own DMA (this wave's
        // share, uniform)
        const bool st = MODE == 1 && k >= 3;
        const int nd = dma ? my_dma : 0;
        if (nd == 0) {
          if (st) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST) : "memory");
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (nd == 1) {
          if (st) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST + 1) : "memory");
          else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        } else {
          if (st) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST + 2) : "memory");
          else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        }
      }
      __syncthreads();  // D complete; every wave's horizontal reads of V are done
      {  // vertical down
        // output column of accumulator i: wave + NW i, or 4 wave + i (BLK).  Either way one read instruction takes one
        // column, so its lanes differ only in (row 4 g + tq, quad tp): the bank pattern D_PITCH was chosen for
        fm_s4 da[OCW];
#pragma unroll
        for (int i = 0; i < OCW; ++i)
          da[i] = fm_tr_read(d_img + (4 * g + tq) * G::D_PITCH + (BLK ? 4 * wave + i : wave + NW * i) * G::D_XP + 2 * tp);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MODE == 0) {
#pragma unroll
          for (int i = 0; i < OCW; ++i)
            acc_b[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(fm_h4, da[i]), gdv[0],
                                                             fm_f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        } else if constexpr (MODE == 1) {
#pragma unroll
          for (int i = 0; i < OCW; ++i)
            acc_a[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(fm_h4, da[i]), gdv[1], acc_b[i], 0, 0, 0);
        } else {
#pragma unroll
          for (int i = 0; i < OCW; ++i)
            acc_a[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(fm_h4, da[i]), gdv[2], acc_a[i], 0, 0, 0);
          if (k < kend) {
#pragma unroll
            for (int i = 0; i < OCW; ++i)
              acc_b[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(fm_h4, da[i]), gdv[0],
                                                               fm_f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };

    block(0, std::integral_constant<int, 0>{}, std::false_type{});
    const int nfull = nt - (tail_skip ? 1 : 0);
    for (int t = 0; t < nfull; ++t) {
      block(2 * t + 1, std::integral_constant<int, 1>{}, std::false_type{});
      block(2 * t + 2, std::integral_constant<int, 2>{}, std::true_type{});
      store_tile(t);
    }
    if (tail_skip) {  // the image's last tile: acc_a is complete after its odd block
      block(kend, std::integral_constant<int, 1>{}, std::true_type{});
      store_tile(nt - 1);
    }
  }
}


// (up, delta) -> template arguments: f(integral_constant<U>, integral_constant<DELTA>), up in {2, 4}, delta < up
template <typename F>
static int fm_dispatch(int up, int delta, F&& f) {
  using std::integral_constant;
  if (up == 2) return delta == 0 ? f(integral_constant<int, 2>{}, integral_constant<int, 0>{})
                                 : f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
  switch (delta) {
    case 0: return f(integral_constant<int, 4>{}, integral_constant<int, 0>{});
    case 1: return f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
    case 2: return f(integral_constant<int, 4>{}, integral_constant<int, 2>{});
    default: return f(integral_constant<int, 4>{}, integral_constant<int, 3>{});
  }
}

template <int U, int DELTA, bool CL, bool BLK>
static void fm3_launch_cl(FlrArgs a, int n, hipStream_t s) {
  constexpr int TOX = FmGeom3<U>::TOX, NW = 8;
  a.tiles_x = (int)ceil_div(a.out_w, TOX);
  a.tiles_y = (int)ceil_div(a.out_h, 16);
  a.cblocks = a.c_p / 16;
  static const int resident = fm_resident(flrelu_mfma3_kernel<U, DELTA, NW, CL, BLK>, 64 * NW);
  // strip segmentation: fm_strip_segments (flrelu_mfma.h); knob IC2_FLR_SEGS=0 keeps the round-3 rule
  static const int segs_mode = knob("IC2_FLR_SEGS", 1);
  const FmStripGrid sg = fm_strip_grid((int64_t)n * a.tiles_x * a.cblocks, a.tiles_y, resident, segs_mode == 1);
  hipLaunchKernelGGL((flrelu_mfma3_kernel<U, DELTA, NW, CL, BLK>), dim3((unsigned)sg.grid), dim3(64 * NW), 0, s, a,
                     sg.nitems, sg.nseg, sg.seg_len);
}

// the clamp-split activation needs a finite clamp whose reciprocal scaling keeps the f16 operands normal
// (lim in [2^-4, 2^12]: SG3's conv_clamp 256 / sqrt(2)); knob IC2_FLR_CLSPLIT=0 keeps the 3-instruction activation.
template <int U, int DELTA>
static int fm3_launch(const FlrArgs& a, int n, hipStream_t s) {
  static const bool split = knob("IC2_FLR_CLSPLIT", 1) != 0;
  const bool cl = split && a.lim >= 0.0625f && a.lim <= 4096.f;
  if (a.out_blocked) {
    if (cl) fm3_launch_cl<U, DELTA, true, true>(a, n, s);
    else fm3_launch_cl<U, DELTA, false, true>(a, n, s);
  } else {
    if (cl) fm3_launch_cl<U, DELTA, true, false>(a, n, s);
    else fm3_launch_cl<U, DELTA, false, false>(a, n, s);
  }
  return IC2_OK;
}

template <int U, int DELTA>
static int fm_launch(const FlrArgs& a, int ntiles, hipStream_t s) {
  // persistent grid: every CU filled to the kernel's occupancy, capped by the tile count
  static const int resident = fm_resident(flrelu_mfma_kernel<U, DELTA>, 256);
  const int grid = ntiles < resident ? ntiles : resident;
  hipLaunchKernelGGL((flrelu_mfma_kernel<U, DELTA>), dim3((unsigned)grid), dim3(256), 0, s, a, ntiles);
  return IC2_OK;
}

int flrelu_mfma_launch(FlrArgs a, int in_f16, int up, int down, int tu, int td, int delta, int n, hipStream_t s) {
  if (down != 2 || td != 12 || tu != 6 * up || (up != 2 && up != 4) || a.bias != nullptr || a.c_p % 16 != 0)
    return IC2_E_UNSUPPORTED;
  if ((int64_t)a.in_h * a.in_w * a.c_p * 2 >= (int64_t)FM_OOB) return IC2_E_UNSUPPORTED;  // 32-bit buffer offsets
  if (a.xsc != 1 || a.xsx % 8 != 0) return IC2_E_UNSUPPORTED;  // 16-B chunks of 8 channels
  if ((int64_t)a.out_h * a.out_w * a.c_p * 2 >= (int64_t)FM_OOB) return IC2_E_UNSUPPORTED;  // output offsets too
  if (in_f16) {  // the synthesis path: the strip kernel
    const int64_t tiles = (int64_t)n * ceil_div(a.out_h, 16) * ceil_div(a.out_w, 32) * (a.c_p / 16);
    if (tiles >= (1LL << 31)) return IC2_E_UNSUPPORTED;
    return fm_dispatch(up, delta, [&](auto u, auto d) {
      return fm3_launch<decltype(u)::value, decltype(d)::value>(a, n, s);
    });
  }
  if (a.out_blocked) return IC2_E_UNSUPPORTED;  // bf16 input: the tile kernel writes NHWC only
  a.tiles_x = (int)ceil_div(a.out_w, 16);
  a.tiles_y = (int)ceil_div(a.out_h, 16);
  a.cblocks = a.c_p / 16;
  const int64_t grid = (int64_t)n * a.tiles_y * a.tiles_x * a.cblocks;
  if (grid >= (1LL << 31)) return IC2_E_UNSUPPORTED;
  return fm_dispatch(up, delta, [&](auto u, auto d) {
    return fm_launch<decltype(u)::value, decltype(d)::value>(a, (int)grid, s);
  });
}

}  // namespace ic2
