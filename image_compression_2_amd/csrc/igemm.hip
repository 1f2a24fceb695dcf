// NHWC implicit-GEMM convolution on CDNA4 MFMA.
//
// Replaces (a) the grouped conv2d inside StyleGAN3's modulated_conv2d [SG3-public; call sites
// /root/reference/stylegan3_hvae_full.py:274,329] in its activation-scaling form, (b) the VGGBlock
// and from_rgb nn.Conv2d of HVAE_VGG_Encoder (stylegan3_hvae_full.py:62,175-176) and (c) the
// 1x1 "x @ W^T" of SynthesisInput.
//
// GEMM view (per launch):  C^T[o][p] = sum_k W[o][k] * X[p][k]
//   o = output channel (MFMA A rows; weights stored [cout_p][kh][kw][cin_p], K-contiguous)
//   p = output pixel over the whole batch (MFMA B cols; NHWC input gives 8 consecutive k per lane)
//   k = (ky, kx, ci) with ci innermost; one K-chunk = 32 channels of one tap.
// Tile BO(o) x BP(p) x 32(k); WGO x WGP waves, each owning (BO/WGO) x (BP/WGP) = I x J MFMA tiles.
//   bf16: v_mfma_f32_16x16x32_bf16 (one MFMA per 16x16 tile per chunk)
//   f32 : v_mfma_f32_16x16x4_f32   (exact fp32 FMA chain; 8 MFMAs per tile per chunk)
// Global -> LDS by LDS-DMA (global_load_lds_dwordx4) into an NSTAGE-deep ring with counted vmcnt
// and raw s_barrier (chunks q+1 .. q+NSTAGE-2 stay in flight across the barrier).  LDS rows are
// XOR-swizzled per 16-B chunk through the SOURCE address (DMA writes lane-linear), the fragment
// reads apply the same XOR (conflict-free for bf16, 2-way for f32).  Out-of-image taps and padded
// output channels read a zero line instead of branching.  Blocks are remapped so consecutive
// logical tiles (which share input rows / weight panels) land on the same XCD's L2.
// Launches that would not fill the chip (the encoder's 16^2 .. 2^2 blocks) split K over gridDim.y:
// each slice stores f32 partial sums in a caller-owned workspace and igemm_splitk_reduce_kernel
// combines them in slice order (deterministic) through the same epilogue.
// This file: the NSTAGE-ring kernel and the split-K combine.  The other kernel families of the conv: igemm8.hip
// (8-phase implicit GEMM), hg4.hip (4-wave halo GEMM), hconv.hip (halo direct conv, ToRGB), wino.hip; the launch plan
// that picks among them: conv_dispatch.hip.
#include "conv_plan.h"

namespace ic2 {

template <bool BF16, int BO, int BP, int WGO, int WGP, int NSTAGE>
struct IgCfg {
  static constexpr int NW = WGO * WGP;
  static constexpr int ESZ = BF16 ? 2 : 4;       // element bytes
  static constexpr int EPC = 16 / ESZ;           // elements per 16-B chunk
  static constexpr int ROWB = 32 * ESZ;          // LDS row bytes (one K-chunk of one row)
  static constexpr int WB = BO * ROWB, XB = BP * ROWB;  // bytes per stage per operand
  static constexpr int NIW_T = WB / 1024, NIX_T = XB / 1024;            // DMA instructions per stage
  static constexpr int NIW = (NIW_T + NW - 1) / NW, NIX = (NIX_T + NW - 1) / NW;  // per wave
  static constexpr int PER = NIW + NIX;          // DMA instructions per wave per chunk
  static constexpr int TO = BO / WGO, TP = BP / WGP;
  static constexpr int I = TO / 16, J = TP / 16;
  static constexpr int STAGEB = WB + XB;
  __device__ static __forceinline__ int swz(int row) { return BF16 ? ((row >> 1) & 3) : ((row >> 1) & 7); }
  __device__ static __forceinline__ int off(int row, int ch) { return row * ROWB + ((ch ^ swz(row)) << 4); }
};

template <bool BF16, int BO, int BP, int WGO, int WGP, int NSTAGE, bool F16 = false>
__global__ void __launch_bounds__(64 * WGO * WGP, 1) igemm_kernel(IgemmArgs a) {
  using C = IgCfg<BF16, BO, BP, WGO, WGP, NSTAGE>;
  constexpr int EPC = C::EPC, ESZ = C::ESZ, I = C::I, J = C::J, NIW = C::NIW, NIX = C::NIX;
  static_assert(C::I >= 1 && C::J >= 1, "wave tile smaller than one MFMA tile");
  static_assert(C::NIW_T >= 1 && C::NIX_T >= 1, "tile smaller than one DMA instruction");
  __shared__ __attribute__((aligned(16))) char lds[NSTAGE * C::STAGEB];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  const int wo_ = wid / WGP, wp_ = wid % WGP;

  const int logical = xcd_remap(blockIdx.x, a.nblocks);
  int o_tile, p_tile;
  tile_coords(logical, a.tiles_o, a.nblocks / a.tiles_o, a.group, o_tile, p_tile);
  const int o0 = o_tile * BO;
  const int m0 = p_tile * BP;

  const char* __restrict__ xg = reinterpret_cast<const char*>(a.x);
  const char* __restrict__ wg = reinterpret_cast<const char*>(a.w);

  // ---- per-lane DMA slots.  Instruction g of an operand fills LDS bytes [g KiB, g+1 KiB): lane l
  // lands on row g*(1024/ROWB) + l/(ROWB/16), physical slot l%(ROWB/16) = logical chunk slot^swz(row).
  // Waves beyond an operand's instruction count repeat its last instruction (identical bytes).
  // X: per-lane base pointer at tap (0,0) of the lane's pixel; a chunk adds a uniform byte offset.
  const char* x_base[NIX];
  int x_oy[NIX], x_ox[NIX], x_seg[NIX];
  const char* w_base[NIW];
  int w_seg[NIW];
  const int hw = a.ho * a.wo;
#pragma unroll
  for (int k = 0; k < NIX; ++k) {
    const int g = min(wid_u + C::NW * k, C::NIX_T - 1);
    x_seg[k] = g * 1024;
    const int off = g * 1024 + lane * 16;
    const int row = off / C::ROWB;
    const int ch = ((off % C::ROWB) >> 4) ^ C::swz(row);
    const int m = m0 + row;
    const bool ok = m < a.M;
    const int mm = ok ? m : 0;
    const int nn = mm / hw;
    const int rem = mm - nn * hw;
    const int oy = rem / a.wo;
    const int ox = rem - oy * a.wo;
    // rows past M get an out-of-range y so every tap reads the zero line
    x_oy[k] = ok ? oy - a.pad : -(1 << 20);
    x_ox[k] = ox - a.pad;
    const int64_t e = ((int64_t)(nn * a.h + x_oy[k]) * a.w_ + x_ox[k]) * a.x_pix + ch * EPC;
    x_base[k] = xg + (ok ? e : 0) * ESZ;
  }
#pragma unroll
  for (int k = 0; k < NIW; ++k) {
    const int g = min(wid_u + C::NW * k, C::NIW_T - 1);
    w_seg[k] = g * 1024;
    const int off = g * 1024 + lane * 16;
    const int row = off / C::ROWB;
    const int chl = ((off % C::ROWB) >> 4) ^ C::swz(row);
    const int o = o0 + row;
    w_base[k] = o < a.cout_p ? wg + (int64_t)o * a.K * ESZ + chl * 16 : nullptr;
  }
  const int CB = a.cin_p >> 5;
  // split-K: slice blockIdx.y of gridDim.y covers the K-chunks [q0, q1)
  const int q0 = (int)((int64_t)a.nq * blockIdx.y / gridDim.y);
  const int q1 = (int)((int64_t)a.nq * (blockIdx.y + 1) / gridDim.y);
  // chunk cursor of the next DMA (uniform): chunk index, its tap (ky, kx) and 32-channel block
  int iq = q0, icb = q0 % CB, ikx = (q0 / CB) % a.kw, iky = (q0 / CB) / a.kw;
  const int64_t xrow = (int64_t)a.w_ * a.x_pix * ESZ;

#define IC2_IG_ISSUE(buf_)                                                                                    \
  {                                                                                                          \
    char* wl_ = lds + (buf_) * C::STAGEB;                                                                    \
    char* xl_ = wl_ + C::WB;                                                                                 \
    const int64_t wq = (int64_t)iq * 32 * ESZ;                                                               \
    const int64_t xq = iky * xrow + ((int64_t)ikx * a.x_pix + ig_xb32(a, icb) * 32) * ESZ;                    \
    _Pragma("unroll") for (int k = 0; k < NIW; ++k) {                                                        \
      const void* ws = w_base[k] ? (const void*)(w_base[k] + wq) : zero_line();                              \
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ws,                     \
                                       (__attribute__((address_space(3))) void*)(wl_ + w_seg[k]), 16, 0, 0); \
    }                                                                                                        \
    _Pragma("unroll") for (int k = 0; k < NIX; ++k) {                                                        \
      const bool ok = (unsigned)(x_oy[k] + iky) < (unsigned)a.h && (unsigned)(x_ox[k] + ikx) < (unsigned)a.w_; \
      const void* xs = ok ? (const void*)(x_base[k] + xq) : zero_line();                                     \
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)xs,                     \
                                       (__attribute__((address_space(3))) void*)(xl_ + x_seg[k]), 16, 0, 0); \
    }                                                                                                        \
    { /* advance (branch-free); past the slice end the last chunk is re-issued (never consumed) */         \
      const int adv = iq + 1 < q1;                                                                           \
      iq += adv;                                                                                             \
      icb += adv;                                                                                            \
      const int wrap = icb == CB;                                                                            \
      icb = wrap ? 0 : icb;                                                                                  \
      ikx += wrap;                                                                                           \
      const int wrap2 = ikx == a.kw;                                                                         \
      ikx = wrap2 ? 0 : ikx;                                                                                 \
      iky += wrap2;                                                                                          \
    }                                                                                                        \
  }

  f32x4 acc[I][J];
#pragma unroll
  for (int i = 0; i < I; ++i)
#pragma unroll
    for (int j = 0; j < J; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s_ = 0; s_ < NSTAGE - 1; ++s_) IC2_IG_ISSUE(s_);

  const int fr = lane & 15;
  const int fh = lane >> 4;

  for (int q = 0; q < q1 - q0; ++q) {
    const int cur = q % NSTAGE;
    if constexpr (NSTAGE == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTAGE - 2) * C::PER) : "memory");
    __builtin_amdgcn_s_barrier();  // chunk q landed for every wave; chunk q-1 fully read
    __builtin_amdgcn_sched_barrier(0);
    const char* wl = lds + cur * C::STAGEB;
    const char* xl = wl + C::WB;
    if constexpr (BF16) {
      // all fragment reads first (B, then A in use order), then the refill of the slot chunk q-1 used
      // (its address math runs under the read latency), then the MFMAs: group i waits only for its
      // own A fragment (counted lgkmcnt), the later reads stay in flight
      bf16x8 bfr[J], af[I];
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int row = wp_ * C::TP + j * 16 + fr;
        bfr[j] = *reinterpret_cast<const bf16x8*>(xl + C::off(row, fh));
      }
#pragma unroll
      for (int i = 0; i < I; ++i) af[i] = *reinterpret_cast<const bf16x8*>(wl + C::off(wo_ * C::TO + i * 16 + fr, fh));
      __builtin_amdgcn_sched_barrier(0);
      IC2_IG_ISSUE((q + NSTAGE - 1) % NSTAGE);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j)
          acc[i][j] = mfma32<F16>(af[i], bfr[j], acc[i][j]);
    } else {
      IC2_IG_ISSUE((q + NSTAGE - 1) % NSTAGE);
      __builtin_amdgcn_sched_barrier(0);
      // lane group fh uses k = 8*fh + s for step s: chunks 2fh (s<4) and 2fh+1 (s>=4)
      f32x4 af[I][2], bfr[J][2];
#pragma unroll
      for (int i = 0; i < I; ++i) {
        const int row = wo_ * C::TO + i * 16 + fr;
        af[i][0] = *reinterpret_cast<const f32x4*>(wl + C::off(row, 2 * fh));
        af[i][1] = *reinterpret_cast<const f32x4*>(wl + C::off(row, 2 * fh + 1));
      }
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int row = wp_ * C::TP + j * 16 + fr;
        bfr[j][0] = *reinterpret_cast<const f32x4*>(xl + C::off(row, 2 * fh));
        bfr[j][1] = *reinterpret_cast<const f32x4*>(xl + C::off(row, 2 * fh + 1));
      }
#pragma unroll
      for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int i = 0; i < I; ++i)
#pragma unroll
          for (int j = 0; j < J; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][s >> 2][s & 3], bfr[j][s >> 2][s & 3], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);  // every MFMA of this chunk before the next wait
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the redundant tail DMAs before exit
#undef IC2_IG_ISSUE

  ig_epilogue<I, J>(a, acc, o0 + wo_ * C::TO, m0 + wp_ * C::TP, fr, fh);
}

// split-K combine: sum the slices in slice order (deterministic), then the epilogue; one thread per
// (pixel, 4 channels)
__global__ void __launch_bounds__(256) igemm_splitk_reduce_kernel(IgemmArgs a, int splits, int p_lo) {
  const int c4 = a.cout_p >> 2;
  const int total = (a.M - p_lo) * c4;  // < 2^31 (checked by the launcher); pixels [p_lo, M) (the split tail)
  const int hw = a.ho * a.wo;
  const int64_t slice = (int64_t)a.M * a.cout_p;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int q = e / c4;
    const int p = p_lo + q;
    const int ob = (e - q * c4) * 4;
    const float* src = a.ws + (int64_t)p * a.cout_p + ob;
    f32x4 s = *reinterpret_cast<const f32x4*>(src);
    for (int k = 1; k < splits; ++k) s += *reinterpret_cast<const f32x4*>(src + k * slice);
    const int nn = p / hw;
    const float v[4] = {s[0], s[1], s[2], s[3]};
    ig_store4(a, p, nn, p - nn * hw, ob, v);
  }
}

template <bool BF16, int BO, int BP, int WGO, int WGP, int NSTAGE, bool F16 = false>
static void launch_tile(IgemmArgs a, int splits, hipStream_t s) {
  a.tiles_o = (a.cout_p + BO - 1) / BO;
  a.nblocks = (int)(ceil_div(a.M, BP) * a.tiles_o);
  hipLaunchKernelGGL((igemm_kernel<BF16, BO, BP, WGO, WGP, NSTAGE, F16>), dim3(a.nblocks, splits),
                     dim3(64 * WGO * WGP), 0, s, a);
}
template <bool F16>
static void launch_tile16(const IgemmArgs& a, int tile, int splits, hipStream_t s) {
  switch (tile) {
    case IG_256x256: launch_tile<true, 256, 256, 2, 4, 4, F16>(a, splits, s); break;
    case IG_32x256: launch_tile<true, 32, 256, 1, 4, 4, F16>(a, splits, s); break;
    case IG_128x256: launch_tile<true, 128, 256, 2, 4, 4, F16>(a, splits, s); break;
    case IG_64x256: launch_tile<true, 64, 256, 1, 4, 4, F16>(a, splits, s); break;
    default: launch_tile<true, 128, 128, 2, 2, 4, F16>(a, splits, s); break;  // IG_128x128
  }
}

void launch_igemm(const IgemmArgs& a, int tile, bool f16, int splits, hipStream_t s) {
  if (tile == IG_F32_128x128) launch_tile<false, 128, 128, 2, 2, 2>(a, splits, s);
  else if (f16) launch_tile16<true>(a, tile, splits, s);
  else launch_tile16<false>(a, tile, splits, s);
}

// the pixels [p_lo, M) of `splits` slices of partial sums (p_lo > 0: the split tail of an 8-phase grid, igemm8.hip)
void launch_splitk_reduce(const IgemmArgs& a, int splits, int p_lo, hipStream_t s) {
  const int64_t total = (int64_t)(a.M - p_lo) * (a.cout_p / 4);
  const int grid = (int)(ceil_div(total, 256) < 4096 ? ceil_div(total, 256) : 4096);
  hipLaunchKernelGGL(igemm_splitk_reduce_kernel, dim3(grid), dim3(256), 0, s, a, splits, p_lo);
}

}  // namespace ic2
