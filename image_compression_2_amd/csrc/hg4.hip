// Halo implicit GEMM, 4-wave form (`hg4`).  The implicit GEMM (igemm.hip) stages a shifted pixel panel per tap, so every
// input pixel crosses L2 -> LDS nine times per channel block; here the output tile is a 2-D block of pixels of one
// sample whose (TH+2) x (TW+2) input halo is staged ONCE per 32-channel block and read at nine shifted offsets.
// An 8-wave form of the same idea (one workgroup per CU, all waves meeting at each K-step barrier: MFMA busy
// 0.30-0.38, round 2) was removed; here a workgroup is 4 waves (one per SIMD) and needs <= 74 KB of LDS, so two
// independent workgroups share each CU and one's barrier / fragment-read phase overlaps the other's MFMAs.
//   K-step = one tap x 32 channels (64-B LDS rows); wave tile (16 I) o x (16 J) px, 2 fragments per MFMA pair
//   read per step: I + J ds_read_b128 for I*J MFMAs (8 + 4 for 32 at the 128 x 256 tile: 12 KB per wave and
//   step).
//   Weights stream through a 3-slab ring (the slab for step t+2 is issued at step t, so a DMA has a whole step
//   plus the barrier to land); the next 32-channel block's halo is spread over the first taps of the current
//   block, one 1-KiB DMA per wave per step, so every step waits for the same small count (vmcnt(NWI [+1])).
//   LDS rows of 64 B, 16-B chunk c stored at c ^ (((row >> 2) & 1) << 1): conflict-free ds_read_b128 for 16
//   consecutive rows starting at ANY row (the halo fragments start at tap-shifted rows), checked by brute force
//   over the four ds_read_b128 lane groups.
#include "conv_plan.h"

namespace ic2 {

template <int I, int J, int WGO, int WGP, int TW, int NS, bool HB = false>
struct H4 {
  static constexpr int BO = 16 * I * WGO, BP = 16 * J * WGP, TH = BP / TW;
  static constexpr int HW = TW + 2, HH = TH + 2, NH = HH * HW;  // halo pixels
  static constexpr int NHI = (NH + 15) / 16;                    // 1-KiB DMA instructions per halo (16 px)
  static constexpr int HPW = (NHI + 3) / 4;                     // per wave, at most
  static constexpr int HALO_B = NHI * 1024;
  static constexpr int WS_B = BO * 64;                          // one weight slab: BO rows x 32 channels
  static constexpr int NWI = (BO / 16 + 3) / 4;                 // weight DMA instructions per wave
  static constexpr int LDS_B = NS * WS_B + 2 * HALO_B + (HB ? 1024 : 0);  // NS-slab weight ring (+ HB dummy slot)
  static_assert(BP % TW == 0 && TW % 16 == 0, "pixel tile");
  // weight slab rows split over the 4 waves: evenly, or (BO = 96) waves 2-3 issue one DMA fewer, which only the
  // one-step lookahead of the multi-tap loop (L = 1: its waits do not count weight DMAs) allows
  static_assert((BO / 16) % 4 == 0 || BO == 96, "weight slab rows over the 4 waves");
  static_assert(HB || HPW <= 8, "halo DMA spread over the first 8 taps");
  static_assert(LDS_B <= 80 * 1024, "two workgroups per CU");
};
__device__ __forceinline__ int h4_off(int row, int chunk) { return row * 64 + ((chunk ^ (((row >> 2) & 1) << 1)) << 4); }

// HB: the next block's halo is issued as one burst at the block's first tap, every wave exactly HPW DMAs (the ones
// past the halo into a 1-KiB dummy slot), so no per-tap selection of a halo-offset register (a uniform branch
// chain, ~60 SALU per step) and a wait count that depends only on the tap
// PAIR (split-weight f16 input, IC2_F16X2, TPB = 2): K blocks cb and cb + CB/2 (x * w_hi, x * w_lo) read the same
// stored channel block, so the steps run tap-major over the pair -- (tap, hi), (tap, lo) share one barrier step and one
// set of halo fragments, and each stored block's halo is loaded once for its 18 steps instead of twice for 9 each
template <int I, int J, int WGO, int WGP, int TW, int NS, bool HB = false, bool F16 = false, int TPB = 1,
          bool GN = false, bool PAIR = false>
__device__ __forceinline__ void hg4_body(const IgemmArgs& a, int tiles_x, int tiles_y) {
  using G = H4<I, J, WGO, WGP, TW, NS, HB>;
  static_assert(!PAIR || (TPB == 2 && HB), "PAIR: two taps per barrier step with the halo burst");
  static_assert((G::BO / 16) % 4 == 0 || (TPB == 2 && NS == 4), "uneven weight DMAs need the L = 1 multi-tap loop");
  constexpr int LA = NS - 1;  // weight slabs in flight ahead of the step being computed
  constexpr int NWI = G::NWI, HPW = G::HPW;
  __shared__ __attribute__((aligned(16))) char lds[G::LDS_B];
  char* const wsl = lds;                    // NS weight slabs
  char* const hal = lds + NS * G::WS_B;     // 2 halos
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int og = wid / WGP, pg = wid % WGP;
  const int fr = lane & 15, fh = lane >> 4;

  const int logical = xcd_remap(blockIdx.x, a.nblocks);
  const int o_tile = logical % a.tiles_o;
  int pt = logical / a.tiles_o;
  const int tx = pt % tiles_x;
  pt /= tiles_x;
  const int ty = pt % tiles_y;
  const int nn = pt / tiles_y;
  const int o0 = o_tile * G::BO;
  const int oy0 = ty * G::TH, ox0 = tx * TW;

  const char* __restrict__ xg = reinterpret_cast<const char*>(a.x);
  const char* __restrict__ wg = reinterpret_cast<const char*>(a.w);
  const int lrow = lane >> 2, pch = lane & 3;  // DMA: 16 rows x 4 chunks of 16 B per instruction

  uint32_t w_off[NWI];
#pragma unroll
  for (int k = 0; k < NWI; ++k) {
    const int row = (wid + 4 * k) * 16 + lrow;
    const int o = o0 + row;
    w_off[k] = (row < G::BO && o < a.cout_p) ? (uint32_t)(o * a.K * 2 + ((pch ^ (((row >> 2) & 1) << 1)) << 4)) : kOob;
  }
  uint32_t h_off[HPW];
#pragma unroll
  for (int k = 0; k < HPW; ++k) {
    const int g = wid + 4 * k;
    const int hp = g * 16 + lrow;
    const int hy = hp / G::HW, hx = hp - (hp / G::HW) * G::HW;
    const int iy = oy0 - a.pad + hy, ix = ox0 - a.pad + hx;
    const bool ok = g < G::NHI && hp < G::NH && (unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w_;
    h_off[k] = ok ? ig_halo_off(a, nn, iy, ix, pch ^ (((hp >> 2) & 1) << 1)) : kOob;
  }
  const int x_cb = 2 * a.x_plane;  // bytes from one stored 32-channel block of the input to the next (64 in NHWC)
  int brow[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int pb = pg * J + j;
    brow[j] = (pb * 16 / TW) * G::HW + (pb * 16) % TW + fr;
  }
  const int obase = og * 16 * I;
  const bool live = o0 + obase < a.cout_p;
  const int CB = a.cin_p >> 5;
  const int nq = CB * 9;
  constexpr int SPB = PAIR ? 18 : 9;    // K-steps per halo block
  const int HBK = PAIR ? CB >> 1 : CB;  // halo blocks
  // K-step t -> (halo block, K block, tap)
  auto step_of = [&](int t, int& hbk, int& cb, int& tap) {
    if constexpr (PAIR) {
      hbk = t / 18;
      const int r = t - hbk * 18;
      tap = r >> 1;
      cb = hbk + (r & 1) * (CB >> 1);
    } else {
      cb = t / 9;
      tap = t - cb * 9;
      hbk = cb;
    }
  };

  auto issue_w = [&](int t) {  // weight slab of K-step t -> slab t % NS
    int hbk_, cb, tap;
    step_of(t, hbk_, cb, tap);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(wg + ((int64_t)tap * a.cin_p + cb * 32) * 2), 0, t < nq ? kOob : 0, kRsrcWord3);
    char* dst = wsl + (t % NS) * G::WS_B;
#pragma unroll
    for (int k = 0; k < NWI; ++k)
      if ((G::BO / 16) % 4 == 0 || wid + 4 * k < G::BO / 16)  // uneven split (BO 96): wave-uniform skip
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs, (__attribute__((address_space(3))) void*)(dst + (wid + 4 * k) * 1024), 16, w_off[k], 0, 0, 0);
  };
  auto issue_hb = [&](int cb) {  // HB: all HPW DMAs of this wave for the halo of block cb -> halo cb & 1 (or dummy)
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(xg + (int64_t)ig_xb32(a, cb) * x_cb), 0, kOob, kRsrcWord3);
#pragma unroll
    for (int k = 0; k < HPW; ++k) {
      char* dst = wid + 4 * k < G::NHI ? hal + (cb & 1) * G::HALO_B + (wid + 4 * k) * 1024 : hal + 2 * G::HALO_B;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, h_off[k], 0, 0, 0);
    }
  };
  auto issue_h1 = [&](int cb, int k) {  // DMA k of this wave for the halo of block cb -> halo cb & 1
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(xg + (int64_t)ig_xb32(a, cb) * x_cb), 0, kOob, kRsrcWord3);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        rs, (__attribute__((address_space(3))) void*)(hal + (cb & 1) * G::HALO_B + (wid + 4 * k) * 1024), 16, h_off[k],
        0, 0, 0);
  };

  f32x4 acc[I][J];
#pragma unroll
  for (int i = 0; i < I; ++i)
#pragma unroll
    for (int j = 0; j < J; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int k = 0; k < HPW; ++k)
    if (wid + 4 * k < G::NHI) issue_h1(0, k);
  if constexpr (TPB > 1) {
    // TPB taps per barrier: step s computes taps TPB*s .. TPB*s+TPB-1 (with TPB = 2 a pair may straddle two channel
    // blocks; both halos are resident).  Slabs of step s+L are issued at step s into the ring positions step s-1
    // read, so the ring holds L+1 steps; the DMA lookahead in MFMA cycles is TPB*L taps (the one-tap ring: LA-1).
    static_assert(HB && NS % TPB == 0 && NS >= 2 * TPB && (TPB == 2 || TPB == 3), "TPB: halo burst, ring of steps");
    constexpr int L = NS / TPB - 1;
    const int nst = (nq + TPB - 1) / TPB;
    auto burst_at = [&](int st) {  // block cb0+1's halo: first step with no tap of block cb0-1
      const int t0 = TPB * st, cb0 = t0 / SPB;
      return t0 - cb0 * SPB < TPB && cb0 + 1 < HBK;
    };
#pragma unroll
    for (int t = 0; t < TPB * L; ++t) issue_w(t);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((L - 1) * TPB * NWI) : "memory");  // halo 0 and step 0's slabs landed
    bf16x8 af[TPB][I], bfr[TPB][J];
    for (int s = 0; s < nst; ++s) {
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      const int t0 = TPB * s;
#pragma unroll
      for (int u = 0; u < TPB; ++u) issue_w(t0 + u + TPB * L);
      const bool burst = burst_at(s);  // first read >= 3 steps later
      if (burst) issue_hb(t0 / SPB + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < TPB; ++u) {
        const int t = t0 + u;
        int hbk, cb, tap;
        step_of(t, hbk, cb, tap);
        // the swizzle depends on the absolute halo row: the tap shift goes into the row, not the base pointer
        const int sh = (tap / 3) * G::HW + tap % 3;
        const char* hb = hal + (hbk & 1) * G::HALO_B;
        const char* wl = wsl + (t % NS) * G::WS_B;
        if (!PAIR || u == 0) {  // PAIR: the step's second K block reads the same halo fragments
#pragma unroll
          for (int j = 0; j < J; ++j) bfr[u][j] = *reinterpret_cast<const bf16x8*>(hb + h4_off(brow[j] + sh, fh));
        }
#pragma unroll
        for (int i = 0; i < I; ++i) af[u][i] = *reinterpret_cast<const bf16x8*>(wl + h4_off(obase + i * 16 + fr, fh));
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      if (live) {
#pragma unroll
        for (int u = 0; u < TPB; ++u) {
          if (u == 0 || t0 + u < nq) {  // the tail step of an odd tap count has one tap
#pragma unroll
            for (int i = 0; i < I; ++i)
#pragma unroll
              for (int j = 0; j < J; ++j) acc[i][j] = mfma32<F16>(af[u][i], bfr[PAIR ? 0 : u][j], acc[i][j]);
          }
        }
      }
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      // step s+1's slabs landed (issued at step s+1-L); a burst of the last L steps may stay in flight (issued after
      // its step's slabs; bursts are >= 3 steps apart)
      const bool recent = burst || (L > 1 && s > 0 && burst_at(s - 1));
      if (recent) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((L - 1) * TPB * NWI + HPW) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((L - 1) * TPB * NWI) : "memory");
    }
  } else {
#pragma unroll
  for (int t = 0; t < LA; ++t) issue_w(t);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"((LA - 1) * NWI) : "memory");  // halo 0 and slab 0 landed
  for (int t = 0; t < nq; ++t) {
    __builtin_amdgcn_s_barrier();  // slab t and block t/9's halo landed for every wave; step t-1's reads done
    __builtin_amdgcn_sched_barrier(0);
    const int cb = t / 9, tap = t - (t / 9) * 9;
    const int ky = tap / 3, kx = tap - (tap / 3) * 3;
    issue_w(t + LA);  // slab (t+LA) % NS was last read by step t-1
    // the next block's halo (halo (cb+1) & 1 was last read by block cb-1): HB one burst at tap 0, else one DMA
    // per step over the block's first taps; wave-uniform conditions
    const bool hdma = !HB && tap < HPW && cb + 1 < CB && wid + 4 * tap < G::NHI;
    if constexpr (HB) {
      if (tap == 0 && cb + 1 < CB) issue_hb(cb + 1);
    } else if (hdma) {
#pragma unroll
      for (int k = 0; k < HPW; ++k)
        if (k == tap) issue_h1(cb + 1, k);
    }
    __builtin_amdgcn_sched_barrier(0);
    const char* wl = wsl + (t % NS) * G::WS_B;
    const char* hl = hal + (cb & 1) * G::HALO_B;
    bf16x8 af[I], bfr[J];
#pragma unroll
    for (int j = 0; j < J; ++j) bfr[j] = *reinterpret_cast<const bf16x8*>(hl + h4_off(brow[j] + ky * G::HW + kx, fh));
#pragma unroll
    for (int i = 0; i < I; ++i) af[i] = *reinterpret_cast<const bf16x8*>(wl + h4_off(obase + i * 16 + fr, fh));
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    if (live) {
#pragma unroll
      for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) acc[i][j] = mfma32<F16>(af[i], bfr[j], acc[i][j]);
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    // slab t+1 (issued at step t+1-LA) landed; the DMAs of the last LA-1 steps may stay in flight (each step
    // issues NWI weight DMAs and, on the block's first taps, one halo DMA; counting the halo DMAs of earlier
    // steps as landed is conservative: vmcnt retires in issue order)
    if constexpr (HB) {  // a burst issued within the last LA-1 steps (tap < LA-1 of a block that issued one)
      if (tap < LA - 1 && cb + 1 < CB) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((LA - 1) * NWI + HPW) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((LA - 1) * NWI) : "memory");
    } else {
      if (hdma) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((LA - 1) * NWI + 1) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((LA - 1) * NWI) : "memory");
    }
  }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the tail (zero-size) DMAs before the epilogue

  const int hw = a.ho * a.wo;
  float4 sc[I], bi[I];  // one sample per tile: every channel block's operands before the first store
#pragma unroll
  for (int i = 0; i < I; ++i) {
    sc[i] = ig_load_oscale(a, nn, o0 + obase + i * 16 + 4 * fh);
    bi[i] = ig_load_bias(a, o0 + obase + i * 16 + 4 * fh);
  }
  ig_preloads_done();
  // GN: 32 groups over cout_p = BO channels; a lane's 4 channels of block i are GL whole groups of CPG
  constexpr int CPG = G::BO / 32, GL = 4 / CPG;
  float gs[GN ? I : 1][GL], gq[GN ? I : 1][GL];  // per-group sums of the stored values over this lane's pixels
  if constexpr (GN) {
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
      for (int r = 0; r < GL; ++r) gs[i][r] = gq[i][r] = 0.f;
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int pb = pg * J + j;
    const int oy = oy0 + pb * 16 / TW, ox = ox0 + (pb * 16) % TW + fr;
    if (oy >= a.ho || ox >= a.wo) continue;
    const int pix = oy * a.wo + ox;
    const int p = nn * hw + pix;
#pragma unroll
    for (int i = 0; i < I; ++i) {
      const int ob = o0 + obase + i * 16 + 4 * fh;
      if (ob >= a.cout_p) continue;
      const float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if constexpr (GN) {
        float st[4];
        ig_store4v(a, p, nn, pix, ob, v, sc[i], bi[i], &st);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gs[i][r / CPG] += st[r];
          gq[i][r / CPG] += st[r] * st[r];
        }
      } else {
        ig_store4v(a, p, nn, pix, ob, v, sc[i], bi[i]);
      }
    }
  }
  if constexpr (GN) {
    // GroupNorm partial sums of this tile: the 16 pixel lanes by an xor tree, the WGP pixel waves of a channel
    // block through LDS, then one thread per group adds the waves in a fixed order in f64 -> gn_part[(nn, g, tile)]
    static_assert(G::BO == 64 || G::BO == 128, "GN epilogue: 2 or 4 channels per group");
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
      for (int r = 0; r < GL; ++r)
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          gs[i][r] += __shfl_xor(gs[i][r], off, 64);
          gq[i][r] += __shfl_xor(gq[i][r], off, 64);
        }
    __syncthreads();  // every wave is past its last LDS fragment read
    float* red = reinterpret_cast<float*>(lds);  // [2][WGP][32 groups]
    if (fr == 0) {
#pragma unroll
      for (int i = 0; i < I; ++i)
#pragma unroll
        for (int r = 0; r < GL; ++r) {
          const int g = (obase + i * 16 + 4 * fh) / CPG + r;
          red[pg * 32 + g] = gs[i][r];
          red[(WGP + pg) * 32 + g] = gq[i][r];
        }
    }
    __syncthreads();
    if (tid < 32) {
      double sg = 0.0, qg = 0.0;
#pragma unroll
      for (int w = 0; w < WGP; ++w) {
        sg += (double)red[w * 32 + tid];
        qg += (double)red[(WGP + w) * 32 + tid];
      }
      double* o = a.gn_part + (((int64_t)nn * 32 + tid) * (tiles_x * tiles_y) + (ty * tiles_x + tx)) * 2;
      o[0] = sg;
      o[1] = qg;
    }
  }
}

#define IC2_HG4_KERNEL(name, I, J, WGO, WGP, TW, NS)                                                             \
  __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) name(IgemmArgs a, int tx,  \
                                                                                          int ty) {            \
    hg4_body<I, J, WGO, WGP, TW, NS>(a, tx, ty);                                                                 \
  }                                                                                                              \
  __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) name##_f16(IgemmArgs a,     \
                                                                                                int tx, int ty) { \
    hg4_body<I, J, WGO, WGP, TW, NS, false, true>(a, tx, ty);                                                    \
  }
// the launch plan's instances: 4-slab one-tap rings for 16-wide pixel tiles, multi-tap halo-burst kernels (below)
// for 32-wide ones
IC2_HG4_KERNEL(hg4_o128_w16_s4_kernel, 8, 4, 1, 4, 16, 4)  // 128 o x (16 x 16) px
IC2_HG4_KERNEL(hg4_o192_w16_s4_kernel, 6, 4, 2, 2, 16, 4)  // 192 o x (8 x 16) px
IC2_HG4_KERNEL(hg4_o64_w16_s4_kernel, 4, 4, 1, 4, 16, 4)   // 64 o x (16 x 16) px
#define IC2_HG4_KERNEL_P(name, I, J, WGO, WGP, TW, NS, TPB)                                                     \
  __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) name(IgemmArgs a, int tx,  \
                                                                                          int ty) {            \
    hg4_body<I, J, WGO, WGP, TW, NS, true, false, TPB>(a, tx, ty);                                               \
  }                                                                                                              \
  __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) name##_f16(IgemmArgs a,     \
                                                                                                int tx, int ty) { \
    hg4_body<I, J, WGO, WGP, TW, NS, true, true, TPB>(a, tx, ty);                                                \
  }
// 32-wide tiles: halo burst + several taps per barrier (two for o96 and for o128, whose 4-slab ring and double
// halo fill the 80 KB; three for o64 with a 6-slab ring, one barrier per kernel row), profiles/r3_hg4_taps_ab.txt
IC2_HG4_KERNEL_P(hg4_o128_w32_p2_kernel, 8, 4, 1, 4, 32, 4, 2)  // 128 o x (8 x 32) px
IC2_HG4_KERNEL_P(hg4_o64_w32_p3_kernel, 4, 4, 1, 4, 32, 6, 3)   // 64 o x (8 x 32) px
IC2_HG4_KERNEL_P(hg4_o96_w32_p2_kernel, 6, 4, 1, 4, 32, 4, 2)   // 96 o x (8 x 32) px
// the split-bf16 encoder's 64- / 128-wide convs with the GroupNorm statistics of their f32 output in the epilogue
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
hg4_o128_w32_p2_gn_kernel(IgemmArgs a, int tx, int ty) {
  hg4_body<8, 4, 1, 4, 32, 4, true, false, 2, true>(a, tx, ty);
}
// 64-wide outputs on 12 x 32-pixel tiles (wave tile 64 x 96: a weight slab feeds 384 pixels, 1.5x the 8-row tile's)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
hg4_o64_w32_t12_gn_kernel(IgemmArgs a, int tx, int ty) {
  hg4_body<4, 6, 1, 4, 32, 4, true, false, 2, true>(a, tx, ty);
}
// the same two with f16 operands: the split encoder's first blocks (IC2_F16X2: f16 input, [hi | lo] f16 weights),
// walking each tap's hi / lo K blocks as one step (PAIR)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
hg4_o128_w32_p2_gn_kernel_f16(IgemmArgs a, int tx, int ty) {
  hg4_body<8, 4, 1, 4, 32, 4, true, true, 2, true, true>(a, tx, ty);
}
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
hg4_o64_w32_t12_gn_kernel_f16(IgemmArgs a, int tx, int ty) {
  hg4_body<4, 6, 1, 4, 32, 4, true, true, 2, true, true>(a, tx, ty);
}
#undef IC2_HG4_KERNEL
#undef IC2_HG4_KERNEL_P

// The plan's instance (h4_plan, conv_dispatch.hip; its th x tw are the kernel's pixel tile), or with gn_stats the
// statistics-epilogue kernel of a 32-wide-tile o64 (12-row tiles) / o128 plan.
// The halo burst on 32-wide tiles (s276a +2.6 %, s276b +3 %, SG3-T-1024 L11 +7 % over spreading the halo DMAs over
// the first taps, profiles/r2f_hg4_hb.txt); a 4-slab weight ring (+0.5-1 % over 3, profiles/r2e_hg4_sweep.txt)
void launch_hg4(IgemmArgs a, const H4Plan& p, bool f16, bool gn_stats, hipStream_t s) {
  void (*kern)(IgemmArgs, int, int);
  if (gn_stats) {
    if (p.bo == 64) kern = f16 ? hg4_o64_w32_t12_gn_kernel_f16 : hg4_o64_w32_t12_gn_kernel;
    else kern = f16 ? hg4_o128_w32_p2_gn_kernel_f16 : hg4_o128_w32_p2_gn_kernel;
  } else if (p.tw32) {
    if (p.bo == 128) kern = f16 ? hg4_o128_w32_p2_kernel_f16 : hg4_o128_w32_p2_kernel;
    else if (p.bo == 96) kern = f16 ? hg4_o96_w32_p2_kernel_f16 : hg4_o96_w32_p2_kernel;
    else kern = f16 ? hg4_o64_w32_p3_kernel_f16 : hg4_o64_w32_p3_kernel;
  } else {
    if (p.bo == 192) kern = f16 ? hg4_o192_w16_s4_kernel_f16 : hg4_o192_w16_s4_kernel;
    else if (p.bo == 128) kern = f16 ? hg4_o128_w16_s4_kernel_f16 : hg4_o128_w16_s4_kernel;
    else kern = f16 ? hg4_o64_w16_s4_kernel_f16 : hg4_o64_w16_s4_kernel;
  }
  const int tiles_x = (int)ceil_div(a.wo, p.tw), tiles_y = (int)ceil_div(a.ho, p.th);
  a.tiles_o = (a.cout_p + p.bo - 1) / p.bo;
  a.nblocks = a.n * tiles_x * tiles_y * a.tiles_o;
  hipLaunchKernelGGL(kern, dim3(a.nblocks), dim3(256), 0, s, a, tiles_x, tiles_y);
}

}  // namespace ic2
