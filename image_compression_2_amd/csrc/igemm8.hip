// 8-phase NHWC implicit-GEMM convolution (the GEMM view, epilogue and tile order of igemm.hip; 2-byte operands only).
// 64-deep K-tiles (64 channels of one tap), 8 waves each owning 128 x 64 outputs:
//   OG = 2: 256 x 256 tile, 2 o-groups x 4 p-groups;
//   OG = 1: 128 x 512 tile (the cout_p <= 128 layers), 1 o-group x 8 p-groups.
// Eight phases per iteration (two K-tiles, LDS double buffer): phase = (ds_read the quadrant's
// fragments, DMA one half-tile, [counted vmcnt], s_barrier, 16 MFMAs at raised priority, s_barrier).
// Waves 4-7 run one barrier behind waves 0-3, so on every SIMD (one wave of each half) one wave's
// MFMAs overlap the other's LDS reads and DMA issue.
//   quadrant per phase&3 : (qm,qn) = (0,0) (0,1) (1,1) (1,0); reads A(qm)+B(qn), B(1), A(1), B(0)
//   half-tile restaged   : ph0 buf1.A1<-t+1  ph1 buf1.B0<-t+1  ph2..5 buf0.{A0,B1,A1,B0}<-t+2
//                          ph6 buf1.A0<-t+3  ph7 buf1.B1<-t+3      (t = 2*iteration)
// Every half is restaged >= 2 phases after its last read (WAR) and read >= 1 phase after the
// vmcnt + barrier that retires it (RAW: the waits in phases 3 and 7 leave only the two newest halves,
// NA + NB DMA instructions, in flight).  Half-tile qm of A = the rows {128*og + 64*qm + [0, 64)};
// half-tile qn of B = the rows {64*pg + 32*qn + [0, 32)}: NA = OG and NB = 4 / OG 1-KiB DMA
// instructions per wave.  LDS rows are 128 B, 16-B chunk c stored at c ^ ((row >> 1) & 7)
// (conflict-free ds_read_b128 for the fragment lane groups).  64-row quadrants lying wholly in the
// o-padding (cout_p 64 / 192 / 384) skip their MFMAs: their accumulators stay 0, which is what those
// rows hold, and the SIMD's partner wave gets the matrix pipe to itself.
#include "conv_plan.h"

namespace ic2 {

template <int OG>
struct G8 {
  static constexpr int BO = 128 * OG, BP = 512 / OG;
  static constexpr int NA = OG, NB = 4 / OG;                    // DMA instructions per wave per half-tile
  static constexpr int BOFF = BO * 128, BUF = (BO + BP) * 128;  // bytes: B offset in a buffer, one buffer
};
__device__ __forceinline__ int g8_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int g8_arow(int qm, int g, int l) { return (g >> 3) * 128 + qm * 64 + (g & 7) * 8 + l; }
__device__ __forceinline__ int g8_brow(int qn, int g, int l) { return (g >> 2) * 64 + qn * 32 + (g & 3) * 8 + l; }

template <int OG, bool F16 = false>
__device__ __forceinline__ void igemm8_body(const IgemmArgs& a) {
  using G = G8<OG>;
  constexpr int NA = G::NA, NB = G::NB;
  __shared__ __attribute__((aligned(16))) char lds[2 * G::BUF];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = wid_u >> 2;                     // waves 4-7 run one barrier behind waves 0-3
  const int grp = OG == 2 ? half : 0;              // o-group
  const int wp_ = OG == 2 ? (wid_u & 3) : wid_u;   // p-group (64 pixels)
  // a launch may cover logical tiles [tile_base, tile_base + gridDim.x) of the a.nblocks-tile grid (the split tail)
  const int logical = a.tile_base + xcd_remap(blockIdx.x, gridDim.x);
  int o_tile, p_tile;
  tile_coords(logical, a.tiles_o, a.nblocks / a.tiles_o, a.group, o_tile, p_tile);
  const int o0 = a.o_base + o_tile * G::BO;  // o_base: a launch covering output channels [o_base, ...) only
  const int m0 = p_tile * G::BP;
  const char* __restrict__ xg = reinterpret_cast<const char*>(a.x);
  const char* __restrict__ wg = reinterpret_cast<const char*>(a.w);

  // per-lane DMA sources: [half][instruction]; instruction k of wave w moves row block g = w + 8k.
  // Buffer loads (raw, stride 0): the per-K-tile part of the address is a scalar descriptor base, the
  // per-lane part a constant 32-bit offset; a tap outside the image / a row past M or cout_p gets the
  // offset kOob (>= num_records), which the hardware answers with zeros.  No per-lane 64-bit math.
  uint32_t w_off[2][NA], x_off[2][NB], x_tap[2][NB];
  const int hw = a.ho * a.wo;
  const int lrow = lane >> 3;                    // row within the 8-row block
  const int pch = lane & 7;                      // physical 16-B chunk written by this lane
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const int ar = g8_arow(h, wid_u + 8 * k, lrow);
      const int o = o0 + ar;
      w_off[h][k] = o < a.cout_p ? (uint32_t)(o * a.K * 2 + ((pch ^ ((ar >> 1) & 7)) << 4)) : kOob;
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int br = g8_brow(h, wid_u + 8 * k, lrow);
      const int m = m0 + br;
      const bool ok = m < a.M;
      const int mm = ok ? m : 0;
      const int nn = mm / hw;
      const int rem = mm - nn * hw;
      const int oy = rem / a.wo;
      const int ox = rem - oy * a.wo;
      // offset of the output pixel's own (oy, ox) position; the descriptor base carries the tap shift
      x_off[h][k] = (uint32_t)((((nn * a.h + oy) * a.w_ + ox) * a.x_pix + ((pch ^ ((br >> 1) & 7)) << 3)) * 2);
      uint32_t mask = 0;
      for (int ky = 0; ky < a.kh; ++ky)
        for (int kx = 0; kx < a.kw; ++kx) {
          const bool in = ok && (unsigned)(oy - a.pad + ky) < (unsigned)a.h && (unsigned)(ox - a.pad + kx) < (unsigned)a.w_;
          mask |= (uint32_t)in << (ky * a.kw + kx);
        }
      x_tap[h][k] = mask;
    }
  }
  const int CB = a.cin_p >> 6;

  // K-tile cursor (uniform): tile index, tap (ky, kx), 64-channel block
  struct Cur {
    int t, ky, kx, cb;
  };
  // K order.  tap-major (cb innermost: K-tile t is the contiguous weight column t) streams a WG's whole
  // 256-pixel x cin_p panel once per tap, so the 9 shifted re-reads of a pixel are cin_p / 64 K-tiles apart and
  // the ~32 resident WGs of an XCD cycle ~8 MB through its 4 MB L2 between them (PMC: 5.4x the compulsory HBM
  // bytes on s148).  channel-major (taps innermost, the halo kernels' order) re-reads each 64-channel panel at the
  // 9 taps back to back: s148 +3 %, s148b +5 %, s148c +7 %, C2 +2.6 % (profiles/r2f_korder.txt), so the host always
  // sets a.korder = 1.  The tap-major arm stays: the kernels measured 1-5 % slower without it
  // (profiles/r11_conv_prune.txt).
  const bool cmaj = a.korder != 0;
  auto advance = [&](Cur c) {
    c.t += 1;
    if (cmaj) {
      c.kx += 1;
      const int wrap = c.kx == a.kw;
      c.kx = wrap ? 0 : c.kx;
      c.ky += wrap;
      const int wrap2 = c.ky == a.kh;
      c.ky = wrap2 ? 0 : c.ky;
      c.cb += wrap2;
    } else {
      c.cb += 1;
      const int wrap = c.cb == CB;
      c.cb = wrap ? 0 : c.cb;
      c.kx += wrap;
      const int wrap2 = c.kx == a.kw;
      c.kx = wrap2 ? 0 : c.kx;
      c.ky += wrap2;
    }
    // the selects above come out as v_cndmask: without this the compiler treats the cursor as divergent and wraps
    // every DMA whose descriptor derives from it in a readfirstlane waterfall loop
    c.t = __builtin_amdgcn_readfirstlane(c.t);
    c.ky = __builtin_amdgcn_readfirstlane(c.ky);
    c.kx = __builtin_amdgcn_readfirstlane(c.kx);
    c.cb = __builtin_amdgcn_readfirstlane(c.cb);
    return c;
  };

#define IC2_G8_ISSUE_A(h_, buf_, c_)                                                                          \
  {                                                                                                          \
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(                                     \
        (void*)(wg + (int64_t)(((c_).ky * a.kw + (c_).kx) * CB + (c_).cb) * 128), 0, (c_).t < t_end ? kOob : 0, \
        kRsrcWord3);                                                                                         \
    _Pragma("unroll") for (int k = 0; k < NA; ++k)                                                           \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lds + (buf_) * G::BUF + \
                                                                                       g8_arow(h_, wid_u + 8 * k, 0) * 128), \
                                               16, w_off[h_][k], 0, 0, 0);                                   \
  }
#define IC2_G8_ISSUE_B(h_, buf_, c_)                                                                          \
  {                                                                                                          \
    const int tap = (c_).ky * a.kw + (c_).kx;                                                                \
    const int64_t sh = ((int64_t)((c_).ky - a.pad) * a.w_ + ((c_).kx - a.pad)) * a.x_pix * 2 +                \
                       ig_xb32(a, 2 * (c_).cb) * 64;                                                          \
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(xg + sh), 0,                  \
                                                                        (c_).t < t_end ? kOob : 0, kRsrcWord3); \
    _Pragma("unroll") for (int k = 0; k < NB; ++k) {                                                         \
      const uint32_t vo = ((x_tap[h_][k] >> tap) & 1u) ? x_off[h_][k] : kOob;                                \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lds + (buf_) * G::BUF + \
                                                                                       G::BOFF + g8_brow(h_, wid_u + 8 * k, 0) * 128), \
                                               16, vo, 0, 0, 0);                                             \
    }                                                                                                        \
  }

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15;
  const int fh = lane >> 4;
  bf16x8 af[4][2], bfr[2][2];
  const int orow = o0 + grp * 128;
  const bool live0 = orow < a.cout_p, live1 = orow + 64 < a.cout_p;

  // split-K (gridDim.y slices, small grids): this workgroup's K-tiles [t_begin, t_end); tiles past t_end come in
  // as zeros (descriptor size 0), so the phase loop needs no tail case
  const int per = (a.nq + (int)gridDim.y - 1) / (int)gridDim.y;
  const int t_begin = __builtin_amdgcn_readfirstlane(min(a.nq, (int)blockIdx.y * per));
  const int t_end = __builtin_amdgcn_readfirstlane(min(a.nq, t_begin + per));
  const int ntap = a.kh * a.kw;
  Cur c0;
  c0.t = t_begin;
  {
    const int tap = cmaj ? t_begin % ntap : t_begin / CB;
    c0.cb = __builtin_amdgcn_readfirstlane(cmaj ? t_begin / ntap : t_begin % CB);
    c0.ky = __builtin_amdgcn_readfirstlane(tap / a.kw);
    c0.kx = __builtin_amdgcn_readfirstlane(tap - (tap / a.kw) * a.kw);
  }

  // prologue: tile 0 -> buf0 (all four halves), tile 1 -> buf1.A0 / buf1.B1 (what phases 6-7 would issue)
  Cur c1 = advance(c0);
  IC2_G8_ISSUE_A(0, 0, c0);
  IC2_G8_ISSUE_B(0, 0, c0);
  IC2_G8_ISSUE_A(1, 0, c0);
  IC2_G8_ISSUE_B(1, 0, c0);
  IC2_G8_ISSUE_A(0, 1, c1);
  IC2_G8_ISSUE_B(1, 1, c1);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NA + NB) : "memory");
  __builtin_amdgcn_s_barrier();
  if (half == 1) __builtin_amdgcn_s_barrier();  // waves 4-7 run one barrier behind
  __builtin_amdgcn_sched_barrier(0);

#define IC2_G8_READ_A(buf_, qm_)                                                                              \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int s = 0; s < 2; ++s) af[i][s] =    \
      *reinterpret_cast<const bf16x8*>(lds + (buf_) * G::BUF + g8_off(grp * 128 + (qm_) * 64 + i * 16 + fr, 4 * s + fh));
#define IC2_G8_READ_B(buf_, qn_)                                                                              \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) _Pragma("unroll") for (int s = 0; s < 2; ++s) bfr[j][s] =   \
      *reinterpret_cast<const bf16x8*>(lds + (buf_) * G::BUF + G::BOFF +                                      \
                                       g8_off(wp_ * 64 + (qn_) * 32 + j * 16 + fr, 4 * s + fh));
#define IC2_G8_COMPUTE(qm_, qn_, WAIT_)                                                                       \
  __builtin_amdgcn_sched_barrier(0);                                                                         \
  WAIT_;                                                                                                     \
  __builtin_amdgcn_s_barrier();                                                                              \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                         \
  __builtin_amdgcn_sched_barrier(0);                                                                         \
  __builtin_amdgcn_s_setprio(1);                                                                             \
  if ((qm_) == 0 ? live0 : live1) {                                                                          \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)             \
        _Pragma("unroll") for (int s = 0; s < 2; ++s) acc[(qm_) * 4 + i][(qn_) * 2 + j] =                    \
            mfma32<F16>(af[i][s], bfr[j][s], acc[(qm_) * 4 + i][(qn_) * 2 + j]);                                   \
  }                                                                                                          \
  __builtin_amdgcn_s_setprio(0);                                                                             \
  __builtin_amdgcn_sched_barrier(0);                                                                         \
  __builtin_amdgcn_s_barrier();                                                                              \
  __builtin_amdgcn_sched_barrier(0);
#define IC2_G8_NOWAIT (void)0
#define IC2_G8_WAIT asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NA + NB) : "memory")

  const int niter = (t_end - t_begin + 1) >> 1;
  Cur cn = c1;  // tile 2i+1
  for (int it = 0; it < niter; ++it) {
    const Cur cA = cn;               // 2i+1
    const Cur cB = advance(cA);      // 2i+2
    const Cur cC = advance(cB);      // 2i+3
    // phase 0: buf0 quadrant (0,0); restage buf1.A1 <- 2i+1
    IC2_G8_READ_B(0, 0);
    IC2_G8_READ_A(0, 0);
    IC2_G8_ISSUE_A(1, 1, cA);
    IC2_G8_COMPUTE(0, 0, IC2_G8_NOWAIT);
    // phase 1: (0,1); buf1.B0 <- 2i+1
    IC2_G8_READ_B(0, 1);
    IC2_G8_ISSUE_B(0, 1, cA);
    IC2_G8_COMPUTE(0, 1, IC2_G8_NOWAIT);
    // phase 2: (1,1); buf0.A0 <- 2i+2
    IC2_G8_READ_A(0, 1);
    IC2_G8_ISSUE_A(0, 0, cB);
    IC2_G8_COMPUTE(1, 1, IC2_G8_NOWAIT);
    // phase 3: (1,0); buf0.B1 <- 2i+2; retire tile 2i+1 (buf1) for phases 4-7
    IC2_G8_READ_B(0, 0);
    IC2_G8_ISSUE_B(1, 0, cB);
    IC2_G8_COMPUTE(1, 0, IC2_G8_WAIT);
    // phase 4: buf1 quadrant (0,0); buf0.A1 <- 2i+2
    IC2_G8_READ_B(1, 0);
    IC2_G8_READ_A(1, 0);
    IC2_G8_ISSUE_A(1, 0, cB);
    IC2_G8_COMPUTE(0, 0, IC2_G8_NOWAIT);
    // phase 5: (0,1); buf0.B0 <- 2i+2
    IC2_G8_READ_B(1, 1);
    IC2_G8_ISSUE_B(0, 0, cB);
    IC2_G8_COMPUTE(0, 1, IC2_G8_NOWAIT);
    // phase 6: (1,1); buf1.A0 <- 2i+3
    IC2_G8_READ_A(1, 1);
    IC2_G8_ISSUE_A(0, 1, cC);
    IC2_G8_COMPUTE(1, 1, IC2_G8_NOWAIT);
    // phase 7: (1,0); buf1.B1 <- 2i+3; retire tile 2i+2 (buf0) for the next iteration
    IC2_G8_READ_B(1, 0);
    IC2_G8_ISSUE_B(1, 1, cC);
    IC2_G8_COMPUTE(1, 0, IC2_G8_WAIT);
    cn = cC;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the tail DMAs (zero tiles) before exit
  if (half == 0) __builtin_amdgcn_s_barrier();      // balance the waves 4-7 offset barrier
#undef IC2_G8_ISSUE_A
#undef IC2_G8_ISSUE_B
#undef IC2_G8_READ_A
#undef IC2_G8_READ_B
#undef IC2_G8_COMPUTE
#undef IC2_G8_NOWAIT
#undef IC2_G8_WAIT
  ig_epilogue<8, 4>(a, acc, orow, m0 + wp_ * 64, fr, fh);
}

// one non-template kernel per instance (a __global__ template's host stub is not emitted here)
__global__ void __launch_bounds__(512, 1) igemm8_og2_kernel(IgemmArgs a) { igemm8_body<2>(a); }
__global__ void __launch_bounds__(512, 1) igemm8_og1_kernel(IgemmArgs a) { igemm8_body<1>(a); }
__global__ void __launch_bounds__(512, 1) igemm8_og2_f16_kernel(IgemmArgs a) { igemm8_body<2, true>(a); }
__global__ void __launch_bounds__(512, 1) igemm8_og1_f16_kernel(IgemmArgs a) { igemm8_body<1, true>(a); }

// tiles [tile_base, tile_base + ntiles) of the grid (ntiles < 0: all of it from tile_base)
template <int OG>
static void launch_g8(IgemmArgs a, bool f16, hipStream_t s, int o_base = 0, int o_end = -1, int splits = 1,
                      int tile_base = 0, int ntiles = -1) {
  a.o_base = o_base;
  a.tiles_o = ((o_end < 0 ? a.cout_p : o_end) - o_base + G8<OG>::BO - 1) / G8<OG>::BO;
  a.nq = a.K / 64;
  a.nblocks = (int)(ceil_div(a.M, G8<OG>::BP) * a.tiles_o);
  a.tile_base = tile_base;
  const unsigned grid = (unsigned)(ntiles < 0 ? a.nblocks - tile_base : ntiles);
  if constexpr (OG == 2)
    hipLaunchKernelGGL(f16 ? igemm8_og2_f16_kernel : igemm8_og2_kernel, dim3(grid, splits), dim3(512), 0, s, a);
  else
    hipLaunchKernelGGL(f16 ? igemm8_og1_f16_kernel : igemm8_og1_kernel, dim3(grid, splits), dim3(512), 0, s, a);
}

void launch_igemm8(const IgemmArgs& a, const ConvPlan& c, bool f16, hipStream_t s) {
  if (c.tile == IG_G8_OG2) {
    if (c.tail) {  // whole rounds at full K, then the tail tiles split over K in two (ig_plan, conv_dispatch.hip)
      launch_g8<2>(a, f16, s, 0, -1, 1, 0, c.tail_tile);
      launch_g8<2>(a, f16, s, 0, -1, 2, c.tail_tile, -1);
    } else {
      launch_g8<2>(a, f16, s, 0, -1, c.splits);
    }
  } else if (c.split384) {  // the 256-wide tile on all but the last 128 channels, the 128 x 512 tile on those
    launch_g8<2>(a, f16, s, 0, a.cout_p - 128, c.splits);
    launch_g8<1>(a, f16, s, a.cout_p - 128, a.cout_p, c.splits);
  } else {
    launch_g8<1>(a, f16, s, 0, -1, c.splits);
  }
}

}  // namespace ic2
