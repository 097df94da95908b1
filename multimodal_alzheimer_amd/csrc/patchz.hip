// Persistent z-walking patch conv for MedicalNet's layer1 (64 -> 64 channels, 3x3x3,
// stride 1, padding 1 on the 32^3 grid of a 128^3 input; pkg/models/mri_models/
// anat_cnn.py:29-31 via MedicalNet's BasicBlock), forward and -- as a forward conv over
// reversed taps -- input gradient, gfx950 bf16 with fp32 accumulation.
//
// patchconv.hip runs one 2x8x8 output box per block and loads its 4x10x10-voxel patch in a
// prologue that nothing overlaps: the round-2 skeleton timings put 54 of its 73 us in that
// prologue, the epilogue and the per-tap barriers.  Here a block stays on one (sample, y
// box, x box) column and walks its z-range in 4x8x8 boxes (256 rows x 64 channels):
//  * the input arrives as 10x10-voxel z-planes (12.8 KiB) through a 6-slot plane ring
//    (plane q in slot q % 6): consecutive boxes share two planes, so each box loads 4 new
//    planes (not 6), and each is loaded over the plane of this box that died last -- 4i+6
//    once the last kz = -1 tap has run (plane 4i is dead), 4i+7 after the last kz = 0 tap,
//    4i+8 and 4i+9 at the box's last barrier; the next box finds them resident;
//  * the taps run in stages of one ky row (the three kx taps) with ONE barrier per stage,
//    9 per box; the weights stream per stage (3 x 8 KiB) through a 3-slot ring, stage G of a
//    box in slot G % 3, two stages ahead, across box boundaries (every box uses the same
//    nine stages).  Inside a stage nothing is overwritten, so the waves drift apart and one
//    wave's fragment reads run beside its SIMD partner's MFMAs;
//  * 8 waves of 32 rows x 64 channels (wave w: z-plane w/2 of the box, y rows 4(w&1)..+3),
//    the 54 half-taps (a tap's 32-channel K halves) of a box pipelined through three
//    fragment register sets: the fragments of half-tap h + 2 are read before the MFMAs of
//    half-tap h, one read in each gap between them, and a stage's barrier stands where
//    stage G + 1's first fragments are read;
//  * the epilogue stages the bf16 box through LDS in two halves (16-byte channel-vector
//    stores) and writes one BN partial-sum row per box.
// LDS: plane ring 6 x 13,312 = 79,872 B | weight ring 3 x 24,576 = 73,728 B | BN sums of the
// 8 waves 4,096 B = 157,696 B.  The half-box output staging (18,432 B) aliases weight slot 2
// (stage 8): dead after the box's last barrier, a DMA target again only at the barrier that
// ends the next box's stage 0.
// Same per-element K order as patchconv.hip (tap-major, channels ascending in 32-wide
// halves), so the conv outputs are bit-identical to it; only the BN partial sums are grouped
// into different rows (one per 4x8x8 box instead of per 2x8x8 box).
#include <type_traits>
#include <utility>

#include "common.h"
#include "patchconv.h"
#include "switches.h"

namespace {

constexpr int PX = 10, PY = 10;                 // plane extent (8 + halo)
constexpr int RB = 128;                         // 64 channels x 2 B per row
constexpr int PROWS = PX * PY;                  // 100
constexpr int PSLOT = 104 * RB;                 // 13 x 1 KiB DMA pieces (rows 100..103 spare)
constexpr int NPS = 6;                          // plane ring slots
constexpr int WSLOT = 64 * RB;                  // one tap's weights: 64 co x 64 ci
constexpr int SSLOT = 3 * WSLOT;                // one stage: the three kx taps of a ky row
constexpr int NST = 3;                          // weight ring slots (two stages in flight)
constexpr int RING_OFF = NPS * PSLOT;           // 79872
constexpr int STG_OFF = RING_OFF + 2 * SSLOT;   // output staging = weight slot 2 (stage 8)
constexpr int CROW = 64 * 2 + 16;               // staged output row (padded)
constexpr int STG_BYTES = 128 * CROW;           // half a box
static_assert(STG_BYTES <= SSLOT, "staging aliases one weight slot");
constexpr int RED_OFF = RING_OFF + NST * SSLOT; // 153600
constexpr int LDS = RED_OFF + 8 * 128 * 4;      // BN sums of waves 0..7
static_assert(LDS <= 160 * 1024, "LDS budget");
constexpr int NTHR = 512, NW = 8;
constexpr int TAPS = 27, STAGES = 9;
constexpr int HT = 2 * TAPS;                    // half-taps (32 input channels each) per box
constexpr int PD = 2;                           // fragment prefetch distance in half-taps
constexpr int NS = PD + 1;                      // fragment register sets (3 x 24 VGPRs)
static_assert(HT % NS == 0 && PD >= 1 && PD < 6, "set of a half-tap is the same in every box");

struct PZ {
  int nb, Nd, Kpad, D, H, W;
  int nty, ntx, nbn, nseg, tps;                 // y / x boxes, channel tiles, z segments,
                                                // boxes per segment
  const u16* res;
  int relu;
};

__device__ const u32x4 g_zero16z[8] = {};
constexpr int EPI_ST = 4;                       // epilogue data stores per wave
constexpr int STATS_ST = 1;                     // BN partial-sum stores (waves 0 and 1)

// counted global stores (see the epilogue): exactly one VMEM instruction each
__device__ __forceinline__ void st_u32x4(void* p, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void st_f32(float* p, float v) {
  asm volatile("global_store_dword %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// LDS hand-over inside the epilogue: this wave's LDS ops done, then the barrier (no vmcnt
// drain, unlike __syncthreads)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// The DMA group issued at the barrier of stage G of a box (the one behind which no wave reads
// stage G any more; it stands where the first fragments of stage G + 1 are read): first the
// weights of stage G + 2 (3 instructions per wave), then -- when a box follows -- its new
// planes (2 instructions each): 1 plane at G = 2 and G = 5, 2 at G = 8.
__host__ __device__ constexpr int planes_at(int g) { return g == 8 ? 2 : (g == 2 || g == 5) ? 1 : 0; }
// VMEM instructions (per wave) younger than the weights of stage G + 1 at the barrier of
// stage G: those weights lead the group of stage G - 1, so only that group's planes (G =
// 0: the previous box's last group, which always has them; the epilogue's stores come on top)
template <int G, bool NEXT>
__host__ __device__ constexpr int younger() {
  return G == 0 ? 2 * planes_at(STAGES - 1) : NEXT ? 2 * planes_at(G - 1) : 0;
}

__global__ __launch_bounds__(NTHR) void patchz_conv_kernel(PZ g, const u16* __restrict__ src,
                                                           const u16* __restrict__ wgt,
                                                           const float* __restrict__ bias,
                                                           u16* __restrict__ dst,
                                                           float* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware order: each XCD walks a contiguous range of work items; neighbouring columns
  // (halo voxels) and the segments of one column meet in one L2
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
  const int item = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
  int t1 = item;
  const int seg = t1 % g.nseg;
  t1 /= g.nseg;
  const int nt = t1 % g.nbn;
  t1 /= g.nbn;
  const int bx = t1 % g.ntx;
  t1 /= g.ntx;
  const int by = t1 % g.nty;
  const int n = t1 / g.nty;
  const int y0 = by * 8, x0 = bx * 8, n0 = nt * 64;
  const int zs = seg * g.tps * 4;               // first output plane of the segment
  const int HW = g.H * g.W;

  // ---- plane DMA: plane q (input z = zs - 1 + q) into slot q % 6; piece p = wave + 8h
  // (13 pieces of 8 rows; surplus pieces repeat piece 12: the same bytes to the same place)
  const u16* __restrict__ srcn = src + (int64_t)n * g.D * HW * 64;
  int poff[2];                                  // lane's voxel offset in the plane (or -1)
  uint32_t pdst[2];
  {
    const int lrow = lane >> 3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int p = min(wave + NW * h, 12);
      const int r = p * 8 + lrow;
      const int px = r % PX, py = r / PX;
      const int y = y0 - 1 + py, x = x0 - 1 + px;
      const bool in = r < PROWS && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W;
      const int chunk = (lane & 7) ^ (px & 7);
      poff[h] = in ? (y * g.W + x) * 64 + chunk * 8 : -1;
      pdst[h] = p * 1024;
    }
  }
  // (x mod 6 for 0 <= x < 12, wave-uniform: one compare and subtract, no division)
  auto mod6 = [](int x) __attribute__((always_inline)) { return x >= NPS ? x - NPS : x; };
  auto issue_plane = [&](int q, int ps) __attribute__((always_inline)) {   // ps = q % 6
    const int z = zs - 1 + q;
    const bool zin = (unsigned)z < (unsigned)g.D;
    const u16* base = srcn + (int64_t)(zin ? z : 0) * HW * 64;
    char* slot = smem + ps * PSLOT;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const void* p = (zin && poff[h] >= 0) ? (const void*)(base + poff[h]) : (const void*)g_zero16z;
      glds16_asm(p, lds_addr_of(slot + pdst[h]));
    }
  };
  // ---- weight DMA: stage G's three 64 x 64 tap slices into slot G % 3, wave w rows 8w ..
  // 8w + 7 of each (three instructions).  A box has 9 stages, so stage and slot are
  // compile-time constants at every call, box after box (a run-time modulo per tap was ~20
  // scalar instructions in the tap loop)
  const int lrow = lane >> 3;
  const u16* wrow = wgt + (int64_t)(n0 + wave * 8 + lrow) * g.Kpad + (((lane & 7) ^ lrow) * 8);
  auto issue_w = [&](auto gc) __attribute__((always_inline)) {
    constexpr int G = decltype(gc)::value;
    static_assert(G >= 0 && G < STAGES);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      glds16_asm(wrow + (3 * G + k) * 64,
                 lds_addr_of(smem + RING_OFF + (G % NST) * SSLOT + k * WSLOT + wave * 1024));
  };

  // ---- fragment addressing: wave w = plane w >> 1 of the box, y rows 4 (w & 1) .. + 3
  const int wz = wave >> 1;
  const int lr = lane & 15, lk = lane >> 4;
  const int tx = lr & 7, ty0 = 4 * (wave & 1) + (lr >> 3);
  uint32_t aoff[3][2];                          // [kx][K half] lane part of the A address
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int k = 0; k < 2; ++k)
      aoff[kx][k] = (uint32_t)((ty0 * PX + tx + kx) * RB + (((4 * k + lk) ^ ((tx + kx) & 7)) << 4));
  uint32_t boff[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) boff[k] = (uint32_t)(lr * RB + (((4 * k + lk) ^ (lr & 7)) << 4));

  f32x4 acc[2][4];
  bf16x8 fa[NS][2], fb[NS][4];                  // fragment sets: half-tap h uses set h % NS
#if defined(PZ_NO_AREAD) || defined(PZ_NO_BREAD)
  // (skeletons: the skipped fragments start as opaque register contents, so the MFMAs stay)
#pragma unroll
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int i = 0; i < 2; ++i) asm volatile("" : "=v"(fa[s][i]));
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "=v"(fb[s][j]));
  }
#endif
  // fragments of K half K of tap T; pslot = byte offset of the ring slot that holds this
  // wave's plane for the tap's kz (wave-uniform, worked out once per box).  The bases go
  // through an opaque scalar so that the compiler does not hoist 54 half-taps' addresses
  // into VGPRs.
  auto read_frags = [&](auto tc, auto kc, int pslot, bf16x8 (&A)[2], bf16x8 (&B)[4])
      __attribute__((always_inline)) {
    constexpr int T = decltype(tc)::value, K = decltype(kc)::value;
    constexpr int ky = (T / 3) % 3, kx = T % 3;
    int pbase = pslot;
    int wbase = RING_OFF + ((T / 3) % NST) * SSLOT + kx * WSLOT;
    asm volatile("" : "+s"(pbase), "+s"(wbase));
    const char* pa = smem + pbase + aoff[kx][K] + ky * PX * RB;
#ifndef PZ_NO_AREAD   // timing skeleton (tools): no A fragment reads (stale registers)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      A[i] = *reinterpret_cast<const bf16x8*>(pa + i * 2 * PX * RB);
#endif
    const char* pb = smem + wbase + boff[K];
#ifndef PZ_NO_BREAD   // timing skeleton (tools): no B fragment reads (stale registers)
#pragma unroll
    for (int j = 0; j < 4; ++j) B[j] = *reinterpret_cast<const bf16x8*>(pb + j * 16 * RB);
#endif
  };
  auto mma = [&](const bf16x8 (&A)[2], const bf16x8 (&B)[4]) __attribute__((always_inline)) {
#ifdef PZ_NO_MMA   // timing skeleton (tools): fragments consumed, no MFMA
#pragma unroll
    for (int i = 0; i < 2; ++i) asm volatile("" ::"v"(A[i]));
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(B[j]));
#else
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[i], B[j], acc[i][j], 0, 0, 0);
#endif
  };

  // ---- epilogue of box i (output planes zs + 4i .. + 3).  No vmcnt drain here: the next
  // box's planes and first weights stay in flight.  Its global stores are VMEM ops too
  // (counted in issue order with the LDS-DMA), so they are issued from asm -- an exact count
  // per wave (EPI_ST; + STATS_ST on waves 0 and 1 when BN sums are written) -- and the
  // first counted wait of the next box (its stage 0, for weights issued before this
  // epilogue) adds them to the younger ops it allows.  The staging area is weight slot 2:
  // every wave is past the box's last barrier, so stage 8 has been read.
  float bv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bv[j] = bias != nullptr ? bias[n0 + j * 16 + lr] : 0.f;
    asm volatile("" ::"v"(bv[j]));              // consumed here: its vmcnt wait comes before
  }                                             // any DMA, not in an epilogue
  const int64_t nbase = (int64_t)n * g.D;
  auto epilogue = [&](int i) __attribute__((always_inline)) {
#ifdef PZ_NO_EPI   // timing skeleton (tools): accumulators consumed, nothing stored
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(acc[a][j]));
    return;
#endif
    const int z0 = zs + 4 * i;
    u16* ctile = reinterpret_cast<u16*>(smem + STG_OFF);
    float cs[4], cq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cs[j] = 0.f;
      cq[j] = 0.f;
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = acc[i2][j][r] + bv[j];
          cs[j] += v;
          cq[j] += v * v;
        }
    }
    // BN partial sums: every wave leaves its 64 sums and 64 sums of squares in LDS; the
    // first staging barrier below hands them over, and waves 0 and 1 add them up, one value
    // per lane.  Then the box in two staged halves.
    float* red = reinterpret_cast<float*>(smem + RED_OFF);
    if (stats != nullptr) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cs[j] += __shfl_xor(cs[j], 16, 64);
        cs[j] += __shfl_xor(cs[j], 32, 64);
        cq[j] += __shfl_xor(cq[j], 16, 64);
        cq[j] += __shfl_xor(cq[j], 32, 64);
      }
      if (lk == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          red[wave * 128 + j * 16 + lr] = cs[j];
          red[wave * 128 + 64 + j * 16 + lr] = cq[j];
        }
      }
    }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      if ((wave >> 2) == hh) {                  // waves 4 hh .. 4 hh + 3 own rows 128 hh ..
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = j * 16 + lr;
#pragma unroll
          for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = (wave & 3) * 32 + i2 * 16 + lk * 4 + r;   // within the half
              ctile[row * (CROW / 2) + col] = f2bf(acc[i2][j][r] + bv[j]);
            }
        }
      }
      lds_barrier();
      if (hh == 0 && stats != nullptr && wave < 2) {
        // lane tid: channel tid & 63 of the sums (wave 0) or the sums of squares (wave 1);
        // waves 0, 1, ..., 7 in order: deterministic, and the bits of a wave-0-first chain
        float s = red[tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[w * 128 + tid];
        const int64_t mt = (((int64_t)n * (g.D / 4) + z0 / 4) * g.nty + by) * g.ntx + bx;
        st_f32(stats + (mt * 2 + wave) * g.Nd + n0 + lane, s);   // one instruction, counted
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {             // 128 rows x 8 chunks / 512 threads
        const int qd = tid + NTHR * h;
        const int row = qd >> 3, c8 = qd & 7;
        const int v = hh * 128 + row;           // box row: z (v >> 6), y, x
        const int64_t vox = ((nbase + z0 + (v >> 6)) * g.H + y0 + ((v >> 3) & 7)) * g.W + x0 + (v & 7);
        const int64_t o = vox * g.Nd + n0 + c8 * 8;
        u32x4 val = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(ctile) +
                                                    row * CROW + c8 * 16);
        if (g.res != nullptr || g.relu) val = epi_res_relu(val, g.res ? g.res + o : nullptr, g.relu);
        st_u32x4(dst + o, val);
      }
      // staging reused by the second half; after that, nothing writes it (or the BN sums)
      // before the barrier that ends the next box's stage 0
      if (hh == 0) lds_barrier();
    }
  };

  // ---- prologue: the first box's six planes, weights of stages 0 and 1
  for (int q = 0; q < NPS; ++q) issue_plane(q, q);
  issue_w(std::integral_constant<int, 0>{});
  issue_w(std::integral_constant<int, 1>{});
  wait_vm_lgkm0<3>();                           // stage 1's weights may still be in flight
  raw_barrier();
  [&]<int... H>(std::integer_sequence<int, H...>) {   // the first PD half-taps' fragments
    (read_frags(std::integral_constant<int, H / 2>{}, std::integral_constant<int, H % 2>{},
                __builtin_amdgcn_readfirstlane(wz * PSLOT), fa[H], fb[H]), ...);
  }(std::make_integer_sequence<int, PD>{});

  // box i, first plane q0 = 4i in ring slot sb = 4i % 6: half-taps unrolled, one barrier per
  // stage; NEXT = a box follows (its planes are issued here), LAST = the segment's last box
  // (no weights past its end)
  auto box = [&](int i, int sb, auto nextc, auto lastc) __attribute__((always_inline)) {
    constexpr bool NEXT = decltype(nextc)::value, LAST = decltype(lastc)::value;
    const int q0 = 4 * i;
    // ring slots of this wave's plane for kz = 0, 1, 2, and for the next box's kz = 0
    int ps[4];
#pragma unroll
    for (int kz = 0; kz < 3; ++kz)
      ps[kz] = __builtin_amdgcn_readfirstlane(mod6(sb + wz + kz) * PSLOT);
    ps[3] = __builtin_amdgcn_readfirstlane(mod6(mod6(sb + 4) + wz) * PSLOT);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[a][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // half-tap H: (at a stage's barrier point: the barrier, then the DMA group;) the
    // fragments of half-tap H + PD; the MFMAs of half-tap H.  The barrier of stage G stands
    // where the first fragments of stage G + 1 are read: every wave has read stage G by then.
    auto half = [&](auto hc) __attribute__((always_inline)) {
      constexpr int H = decltype(hc)::value;
      constexpr int G = H / 6;                  // stage: kz = G / 3, ky = G % 3
      if constexpr (H % 6 == 6 - PD && !(LAST && G == STAGES - 1)) {
        // the weights of stage G + 1 landed (the planes it reads are older)
        constexpr int Y = younger<G, NEXT>();
        if constexpr (G == 0) {                 // the previous box's epilogue stores are
          if (i == 0) {                         // younger than the awaited weights
            wait_vm_lgkm0<0>();
          } else if (wave < 2 && stats != nullptr) {
            wait_vm_lgkm0<Y + EPI_ST + STATS_ST>();
          } else {
            wait_vm_lgkm0<Y + EPI_ST>();
          }
        } else {
          wait_vm_lgkm0<Y>();
        }
#ifndef PZ_NO_BAR   // timing skeleton (tools): no per-stage barrier (races; timing only)
        raw_barrier();
#endif
        // weights first, then planes: the next wait is for these weights
        if constexpr (!(LAST && G + 2 >= STAGES))
          issue_w(std::integral_constant<int, (G + 2) % STAGES>{});
        if constexpr (NEXT && G == 2) {         // over plane q0: its last reader was kz = 0
          issue_plane(q0 + 6, sb);
        } else if constexpr (NEXT && G == 5) {  // over q0 + 1 (sb is 0, 2 or 4)
          issue_plane(q0 + 7, sb + 1);
        } else if constexpr (NEXT && G == 8) {  // over q0 + 2 and q0 + 3
          issue_plane(q0 + 8, mod6(sb + 2));
          issue_plane(q0 + 9, mod6(sb + 3));
        }
      } else if constexpr (H % 6 == 6 - PD && LAST && G == STAGES - 1) {
        lds_barrier();                          // stage 8 read by all: its slot is the staging
      }
      constexpr int N = H + PD;                 // (past the box: the next box's first ones)
      if constexpr (N < HT)
        read_frags(std::integral_constant<int, N / 2>{}, std::integral_constant<int, N % 2>{},
                   ps[N / 18], fa[N % NS], fb[N % NS]);
      else if constexpr (!LAST)
        read_frags(std::integral_constant<int, (N - HT) / 2>{},
                   std::integral_constant<int, (N - HT) % 2>{}, ps[3], fa[N % NS], fb[N % NS]);
      mma(fa[H % NS], fb[H % NS]);
      // issue order: the fragment reads between the MFMAs, one a gap, not in a burst behind
      // them (the set they fill was last used a half-tap ago); the LDS array then runs
      // beside the MFMA pipe, and the SIMD partner's reads find it less often taken
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // 1 LDS read
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    };
    [&]<int... H>(std::integer_sequence<int, H...>) {
      (half(std::integral_constant<int, H>{}), ...);
    }(std::make_integer_sequence<int, HT>{});
    epilogue(i);
  };
  int sb = 0;
  for (int i = 0; i + 1 < g.tps; ++i) {
    box(i, sb, std::true_type{}, std::false_type{});
    sb = sb >= 2 ? sb - 2 : sb + 4;             // + 4 mod 6
  }
  box(g.tps - 1, sb, std::false_type{}, std::true_type{});
}

// z segments per column: the fewest that give every CU a work item, each >= 2 boxes
int segments(const mmad_patch::Geo& q) {
  const int64_t cols = (int64_t)q.nb * (q.Hd / 8) * (q.Wd / 8) * (q.Nd / 64);
  const int boxes = q.Dd / 4;
  int s = 1;
  while (cols * s < 256 && boxes % (2 * s) == 0 && boxes / (2 * s) >= 2) s *= 2;
  return s;
}

}  // namespace

namespace mmad_patchz {

bool ok(const mmad_patch::Geo& q) {
  if (sw(SW_PATCHZ) <= 0) return false;
  if (q.Cs != 64 || q.Nd % 64 || q.Kpad < 27 * 64) return false;
  if (q.KD != 3 || q.KH != 3 || q.KW != 3 || q.dd != 1 || q.dh != 1 || q.dw != 1) return false;
  if (q.pd != 1 || q.ph != 1 || q.pw != 1) return false;
  if (q.Ds != q.Dd || q.Hs != q.Hd || q.Ws != q.Wd) return false;
  if (q.Dd % 4 || q.Hd % 8 || q.Wd % 8) return false;
  const int s = segments(q);
  if (q.Dd / 4 / s < 2) return false;           // nothing to walk
  const int64_t cols = (int64_t)q.nb * (q.Hd / 8) * (q.Wd / 8) * (q.Nd / 64);
  if (sw(SW_PATCHZ) == 1 && cols * s < 256) return false;   // fewer items than CUs
  // per-sample offsets in 32 bits (plane DMA lane offsets, epilogue)
  return (int64_t)q.Ds * q.Hs * q.Ws * 64 < (int64_t(1) << 31) &&
         (int64_t)q.nb * q.Dd * q.Hd * q.Wd * q.Nd < (int64_t(1) << 40);
}

int64_t tiles(const mmad_patch::Geo& q) {
  return (int64_t)q.nb * (q.Dd / 4) * (q.Hd / 8) * (q.Wd / 8);
}

int fwd(const mmad_patch::Geo& q, const void* src, const void* wp, const float* bias, void* dst,
        float* stats, void* stream) {
  if (!mmad_patchz::ok(q)) return MMAD_EUNSUPPORTED;
  if (q.bny != nullptr) return MMAD_EUNSUPPORTED;   // no BN-sum epilogue in this kernel
  static const bool attr =
      hipFuncSetAttribute((const void*)patchz_conv_kernel,
                          hipFuncAttributeMaxDynamicSharedMemorySize, LDS) == hipSuccess;
  if (!attr) return MMAD_EUNSUPPORTED;
  PZ g{};
  g.nb = q.nb; g.Nd = q.Nd; g.Kpad = q.Kpad; g.D = q.Dd; g.H = q.Hd; g.W = q.Wd;
  g.nty = q.Hd / 8; g.ntx = q.Wd / 8; g.nbn = q.Nd / 64;
  g.nseg = segments(q);
  g.tps = q.Dd / 4 / g.nseg;
  g.res = reinterpret_cast<const u16*>(q.res);
  g.relu = q.relu;
  const int64_t items = (int64_t)q.nb * g.nty * g.ntx * g.nbn * g.nseg;
  hipLaunchKernelGGL(patchz_conv_kernel, dim3((unsigned)items), dim3(NTHR), LDS,
                     as_stream(stream), g, (const u16*)src, (const u16*)wp, bias, (u16*)dst,
                     stats);
  return launch_status();
}

}  // namespace mmad_patchz
