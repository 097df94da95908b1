// Residue-class ("lattice") conv, plane-pair form: layer4's dilation-4 3x3x3 convs
// (16^3 grid, 4^3 sub-lattices) forward and -- over reversed taps -- input gradient, gfx950
// bf16 with fp32 accumulation.  Same arithmetic and data layouts as latticeconv.hip
// (packed weights [Nd][27 * Cs], k = tap * Cs + ci; BN partial sums one row per tile);
// what changes is the tile, so that every CU gets the same work and every SIMD runs one
// wave with its accumulators in AGPRs:
//  * latticeconv.hip's tile is one z-plane of 32 subs; the planes at the sub-lattice's
//    z-edges have one kz tap in the padding, so half the tiles carry 2/3 of the work of the
//    others and, at one tile per CU, their CUs idle for a third of the launch.  Here a tile
//    is TWO neighbouring z-planes (tz0 = 0 or 2) of 16 subs: every tile holds one edge plane
//    and one interior plane, 5 of the 6 (plane, kz) pairs -- equal work everywhere;
//  * 8 waves (two per SIMD): wave (wm, wn) owns the positions of the 4 x 4 plane's
//    diagonal wm in BOTH planes (8 fragments of 16 subs = 128 rows) x 64 output channels
//    (TN = 4 16-column MFMA tiles; TN = 2 for 64-channel tiles).  Diagonals lose different
//    numbers of fragments to (y, x) padding (26 / 25 / 24 / 25 of 36 position-taps), but
//    waves w and w + 4 share a SIMD (waves go to SIMDs in a cyclic order of 4) and hold
//    diagonals wm and wm + 2, whose sums are equal on every ky row: every SIMD carries the
//    same MFMA work between two barriers;
//  * fragment registers roll: each A fragment register is refilled for the next tap right
//    after the current tap's MFMAs read it (one A set and two B sets live, ~190 VGPRs with
//    the 128 accumulators) -- a full second fragment set made the compiler shuffle
//    accumulators (one wave per SIMD with 256 accumulators in AGPRs fared worse still: the
//    MFMA results rotate through registers and spill the overflow to VGPRs);
//  * a stage = (channel chunk, kz, ky): the three kx taps' weights (3 x BW rows x 64 B)
//    through a 4-slot ring, three stages in flight; both output planes use the same kz
//    weights, so every B fragment feeds 8 A fragments of the wave (16 of the SIMD pair);
//    the stage loop is software-pipelined across its barriers (see run_pipe);
//  * input planes (16 subs x 16 positions x 32 channels = 16 KiB) through a 4-slot ring:
//    per chunk the pair reads 3 real planes (tz0 - 1 .. tz0 + 2 minus the padding one), each
//    loaded once and read by every kz whose shift lands on it; planes of the next chunk
//    stream in 3 to 9 stages ahead;
//  * padding taps are skipped per fragment at compile time (wave diagonal, plane pair and
//    tap are template constants in the main loop), as in latticeconv.hip.
#include <type_traits>
#include <utility>

#include "bnsum.h"
#include "common.h"
#include "patchconv.h"
#include "switches.h"

namespace {

constexpr int S = 4;                      // sub-lattice extent
constexpr int NS = 16;                    // subs (sample x class) per tile
constexpr int PP = S * S * NS;            // rows per plane: 256
constexpr int RBL = 64;                   // bytes per LDS row: 32 bf16 channels
constexpr int KC = RBL / 2;
constexpr int ZPL = PP * RBL;             // 16 KiB per plane
constexpr int NPS = 4;                    // plane ring slots
constexpr int TPS = 3;                    // taps per stage
// weight ring slots: the pipelined loop keeps NSTL - 1 stages of weights in flight behind
// the one being read.  4 (the default since round 4: +0.8 % on the config-2 step against 3,
// four interleaved bench runs, gpurun_out/r04e) fills the LDS exactly at TN 4: 4 planes + 4
// weight stages = 160 KiB
#ifndef ZP_NSTL
#define ZP_NSTL 4
#endif
constexpr int NSTL = ZP_NSTL;
constexpr int NTHR = 512;
constexpr int NW = NTHR / 64;
constexpr int ROWS = 2 * PP;              // tile rows: 512

template <int TN>
struct ZC {
  static constexpr int BW = 32 * TN;               // output channels per tile
  static constexpr int BTAP = BW * RBL;
  static constexpr int BSLOT = TPS * BTAP;
  static constexpr int RING_OFF = NPS * ZPL;
  static constexpr int MAIN = RING_OFF + NSTL * BSLOT;
  static constexpr int CROW = BW * 2 + 16;
  static constexpr int EPI = ROWS * CROW + 3 * 2 * BW * 4;
  static constexpr int LDS = MAIN > EPI ? MAIN : EPI;
  static constexpr int NQ = TPS * BW / 16;          // weight DMA instructions per stage
  // ... per wave: the same count on every wave (surplus slots repeat the last rows: the
  // same bytes to the same place), so the counted vmcnt waits hold on every wave
  static constexpr int WI = (NQ + NW - 1) / NW;
};

struct ZG {
  int Cs, Nd, Kpad, nchunk, nbn;
  int xcd2;                                 // two channel tiles per XCD (see the tile map)
  const u16* res;
  int relu;
  const u16* bny;                           // dgrad: BN-backward sums epilogue (bnsum.h)
  const float *bnsc, *bnsh, *bnmu, *bnis;
  float* bnparts;
};

__device__ __forceinline__ int swz(int row) { return 3 * ((row >> 3) & 1); }

// position i (row y = i) of diagonal D in the 4 x 4 plane, shifted by (KY, KX): inside?
template <int D, int KY, int KX>
__device__ constexpr bool yx_ok(int i) {
  return i + KY >= 0 && i + KY < S && ((i + D) & 3) + KX >= 0 && ((i + D) & 3) + KX < S;
}
// output plane L (0, 1) of pair P reads input plane tz0 + L + KZ: inside the sub-lattice?
template <int P, int L, int KZ>
__device__ constexpr bool z_ok() {
  return 2 * P + L + KZ >= 0 && 2 * P + L + KZ < S;
}
// ring index (0..2) of the input plane output plane L reads at KZ, among the pair's three
// real planes of a chunk (pair 0 reads absolute planes 0..2, pair 1 planes 1..3)
template <int P, int L, int KZ>
__device__ constexpr int plane_idx() {
  return 2 * P + L + KZ - (P == 0 ? 0 : 1);
}

// A fragment (L, i) of tap (KY, KX): is it inside the sub-lattice (y, x and z)?
template <int WM, int P, int KZ, int KY, int KX, int L, int I>
__device__ constexpr bool frag_ok() {
  return z_ok<P, L, KZ>() && yx_ok<WM, KY, KX>(I);
}
template <int WM, int I, int KY, int KX>
__device__ constexpr int frag_pos() {
  return (I + KY) * S + ((I + WM) & 3) + KX;
}
constexpr int NF = 8;                     // A fragments per wave: 2 planes x 4 positions
// timing skeletons (wrong results): 1 = only the kx = -1 A fragments are read, 2 = no A
// reads, 3 = no A / B reads and no stage waits or barriers
#ifndef ZP_SKEL
#define ZP_SKEL 0
#endif

template <int TN, int KX>
__device__ __forceinline__ void read_b(const char* bsl, bf16x8 (&b)[TN]) {
#if ZP_SKEL >= 3
  return;
#endif
#pragma unroll
  for (int j = 0; j < TN; ++j)
    b[j] = *reinterpret_cast<const bf16x8*>(bsl + (KX + 1) * ZC<TN>::BTAP + j * 16 * RBL);
}

// fragment F = L * 4 + I of tap (KY, KX), if inside, into a[F]
template <int WM, int P, int KZ, int KY, int KX, int F>
__device__ __forceinline__ void read_a(const char* const (&pl)[3], bf16x8 (&a)[NF]) {
  constexpr int L = F / 4, I = F % 4;
  // ZP_SKEL 1 (timing skeleton, wrong results): only the kx = -1 fragments are read
  if constexpr (frag_ok<WM, P, KZ, KY, KX, L, I>() && (ZP_SKEL != 1 || KX == -1) &&
                ZP_SKEL < 2) {
    constexpr int ps = frag_pos<WM, I, KY, KX>();
    a[F] = *reinterpret_cast<const bf16x8*>(pl[plane_idx<P, L, KZ>()] + ps * 16 * RBL);
  }
}

template <int TN, int WM, int P, int KZ, int KY, int KX, int F>
__device__ __forceinline__ void mma_a(f32x4 (&acc)[NF][TN], const bf16x8 (&a)[NF],
                                      const bf16x8 (&b)[TN]) {
  constexpr int L = F / 4, I = F % 4;
  if constexpr (frag_ok<WM, P, KZ, KY, KX, L, I>()) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
      acc[F][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[F], b[j], acc[F][j], 0, 0, 0);
  }
}

// ZP_PIN 1: a scheduling barrier after each fragment's (MFMAs, refill) pair keeps the
// compiler from hoisting the refills (their latency is covered by the other fragments'
// MFMAs anyway) and so from inflating the live fragment registers into spills
#ifndef ZP_PIN_MODE
#define ZP_PIN_MODE 1
#endif
#if ZP_PIN_MODE
#define ZP_PIN() __builtin_amdgcn_sched_barrier(0)
#else
#define ZP_PIN() (void)0
#endif
// planes issued at chunk-relative stage r of a non-last chunk (pair p): count
__host__ __device__ constexpr int planes_at_rt(int p, int r) {
  return p == 0 ? (r == 0 ? 2 : r == 6 ? 1 : 0) : (r == 0 || r == 3 || r == 6 ? 1 : 0);
}
// VMEM ops of DMA group rg (issued after stage rg's barrier) of a chunk with / without a
// successor (pipelined loop): the weights of stage rg + NSTL (while one exists) + planes
__host__ __device__ constexpr int zp_group_ops(int p, int rg, bool more, int wi, int pi) {
  const int pl = more ? planes_at_rt(p, rg) : ((p == 0 && rg == 0) ? 1 : 0);
  return ((more || rg + NSTL < 9) ? wi : 0) + pi * pl;
}
// at stage R's barrier each wave waits for the weights of stage R + 1; younger than them are
// the DMA groups of the NSTL - 2 stages before R (in the first chunk, where those do not
// exist, the prologue's weights of the later stages)
__host__ __device__ constexpr int zp_younger(int p, int r, bool more, bool first, int wi, int pi) {
  int n = 0;
  for (int d = 1; d <= NSTL - 2; ++d) {
    const int g = r - d;
    if (g >= 0) n += zp_group_ops(p, g, more, wi, pi);
    else if (first) n += wi;
    else n += zp_group_ops(p, g + 9, true, wi, pi);
  }
  return n;
}

// BNS: the dgrad epilogue with the BN-backward sums (g.bny set) -- its own instantiation, so
// the plain kernels keep their register allocation (compiled into one body, the BN-sum path
// pushed the stage loops of two wave variants into in-loop scratch reloads, each of which
// waits out every DMA in flight)
template <int TN, bool BNS>
__global__ __launch_bounds__(NTHR) void lattice_zp_kernel(ZG g, const u16* __restrict__ src, const u16* __restrict__ wgt,
                       const float* __restrict__ bias, u16* __restrict__ dst,
                       float* __restrict__ stats) {
  using C = ZC<TN>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem + C::RING_OFF;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
  int nt, t2;
  if (g.xcd2) {
    // two channel tiles per XCD (nbn = 4, sets % 4 == 0, nwg % 8 == 0): XCD x takes channel
    // tiles 2 (x & 1), +1 of a quarter (x >> 1) of the (group, pair) sets, so each XCD's L2
    // pulls half the weights (not all of them) and every input plane is fetched by two XCDs
    // (not one): ~160 MB per launch for layer4.0.conv2 at batch 8 instead of 186
    const int li = bid >> 3, nsets = nwg / g.nbn;
    nt = 2 * (xcd & 1) + (li & 1);
    t2 = (xcd >> 1) * (nsets / 4) + (li >> 1);
  } else {
    const int tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
    nt = tile % g.nbn;                              // channel tile fastest: the tiles of one
    t2 = tile / g.nbn;                              // (group, pair) share their input planes
  }
  const int pair = t2 & 1, gid = t2 >> 1;
  const int n = gid >> 2, rz = gid & 3;             // 64 classes = 4 groups of 16: rz fixed
  constexpr int E = 16, PV = 4 * E * E;             // grid extent; voxels per plane step
  const int tz0 = 2 * pair;
  const int n0 = nt * C::BW;

  // ---- plane DMA: instruction k of wave w = position 2w + k, lane >> 2 = sub, lane & 3 =
  // 16-byte chunk (swizzled); sub s = class rz*16 + s -> (ry, rx) = (s >> 2, s & 3)
  constexpr int PI = 16 / NW;                       // plane DMA instructions per wave
  const u16* __restrict__ srcn = src + (int64_t)n * E * E * E * g.Cs;
  uint32_t pofs[PI];
  {
    const int s = lane >> 2, ry = s >> 2, rx = s & 3;
#pragma unroll
    for (int k = 0; k < PI; ++k) {
      const int pos = wave * PI + k, ty = pos >> 2, tx = pos & 3;
      const int row = pos * NS + s;
      const int vox = (rz * E + ry + 4 * ty) * E + rx + 4 * tx;
      pofs[k] = (uint32_t)(vox * g.Cs + ((lane & 3) ^ swz(row)) * 8);
    }
  }
  // plane jj (0..2) of chunk c -> ring slot (3c + jj) & 3; absolute plane z
  auto issue_plane = [&](int c, int jj) {
    const int z = jj + (pair == 0 ? 0 : 1);
    const u16* base = srcn + (int64_t)z * PV * g.Cs + c * KC;
    char* pb = smem + ((3 * c + jj) & 3) * ZPL;
#pragma unroll
    for (int k = 0; k < PI; ++k) {
      // (opaque lane offset: otherwise the compiler keeps every DMA's 64-bit lane address
      // live across the chunk loop, and the extra VGPRs spill -- a scratch reload in the loop
      // waits out every DMA in flight)
      uint32_t o = pofs[k];
      asm volatile("" : "+v"(o));
      glds16_asm(base + o, lds_addr_of(pb + (wave * PI + k) * 1024));
    }
  };
  // ---- weight DMA: stage (chunk c, kz, ky) -> taps t0 .. t0 + 2 into ring slot sl;
  // instruction q = wave + NW h: tap q / (BW/16), rows 16 * (q % (BW/16)) ..
  uint32_t wofs[C::WI];
  int wq_off[C::WI];
#pragma unroll
  for (int h = 0; h < C::WI; ++h) {
    const int q = min(wave + NW * h, C::NQ - 1);
    const int tk = q / (C::BW / 16), rb = q % (C::BW / 16);
    const int row = rb * 16 + (lane >> 2);
    wofs[h] = (uint32_t)((n0 + row) * g.Kpad + (((lane & 3) ^ swz(row)) * 8) + tk * g.Cs);
    wq_off[h] = tk * C::BTAP + rb * 1024;
  }
  const int nstage = g.nchunk * 9;
  // (stage s = 9 c + r; the callers pass c and r, known up to c at compile time, so the
  // stage loop has no run-time division by 9; slot = s % NSTL)
  auto issue_stage_b = [&](int c, int r, int slot) {
    const u16* base = wgt + (r * 3) * g.Cs + c * KC;   // taps (kz,ky) row: t0 = 3 r
    char* sb = ring + slot * C::BSLOT;
#pragma unroll
    for (int h = 0; h < C::WI; ++h) {
      uint32_t o = wofs[h];
      asm volatile("" : "+v"(o));
      glds16_asm(base + o, lds_addr_of(sb + wq_off[h]));
    }
  };

  // waves w and w + 4 share a SIMD: give them diagonals wm and wm + 2
  const int wn = wave & 1, wm = wave >> 1;
  const int lr = lane & 15, lk = lane >> 4;
  const uint32_t a_lane = lr * RBL + ((lk ^ swz(lr)) << 4);
  const uint32_t b_lane = (wn * 16 * TN + lr) * RBL + ((lk ^ swz(lr)) << 4);
  f32x4 acc[NF][TN];                                // [L * 4 + i][j]
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: the first chunk's planes needed before its plane issues (pair 0: planes 0, 1;
  // pair 1: all three), then the weights of the first NSTL stages
  issue_plane(0, 0);
  issue_plane(0, 1);
  if (pair == 1) issue_plane(0, 2);
  for (int t = 0; t < NSTL; ++t) issue_stage_b(t / 9, t % 9, t % NSTL);

  // The stage loop: the stage boundary is one more step of the rolling pipeline.  Stage s's
  // barrier sits between its kx = 0 and kx = +1 taps: before it each wave waits for the
  // weights of stage s + 1 (and every LDS read of stage s); after it the DMA group of stage
  // s goes out (its planes and the weights of stage s + 3 into stage s's weight slot, free
  // now) and each fragment register, once the kx = +1 MFMAs have read it, is refilled with
  // stage s + 1's kx = -1 fragment.  The MFMA pipe then runs straight across stage
  // boundaries: no wave waits on its first fragment reads after a barrier.  A plane first
  // read by stage t is issued in a DMA group <= t - 3, before the weights of stage t, so the
  // wait at barrier t - 1 covers it; a slot is refilled in group s only when its last reader
  // is stage s or earlier.  Plane issue schedule per chunk c (stage R = 3 (kz+1) + ky+1; slot
  // reuse checked against each plane's last reader):
  //   pair 0: R 0 -> (c, 2), (c + 1, 0); R 6 -> (c + 1, 1)
  //   pair 1: R 0 -> (c + 1, 0); R 3 -> (c + 1, 1); R 6 -> (c + 1, 2)
  auto run_pipe = [&](auto wmc, auto pc) {
    constexpr int WM = decltype(wmc)::value, P = decltype(pc)::value;
    bf16x8 a[NF], b0[TN], b1[TN];
    wait_vm_lgkm0<(NSTL - 1) * C::WI>();            // stage 0's weights and chunk 0's planes
    raw_barrier();
    {
      const char* const pl0[3] = {smem + 0 * ZPL + a_lane, smem + 1 * ZPL + a_lane,
                                  smem + 2 * ZPL + a_lane};
      read_b<TN, -1>(ring + b_lane, b0);
      [&]<int... F>(std::integer_sequence<int, F...>) {
        (read_a<WM, P, -1, -1, -1, F>(pl0, a), ...);
      }(std::make_integer_sequence<int, NF>{});
    }
    // the last chunk is its own instantiation (MORE = false), so that no stage carries a
    // run-time branch between its MFMAs
    auto chunk = [&](int c, auto morec) {
      constexpr bool MORE = decltype(morec)::value;
      const char* const pl[3] = {smem + ((3 * c + 0) & 3) * ZPL + a_lane,
                                 smem + ((3 * c + 1) & 3) * ZPL + a_lane,
                                 smem + ((3 * c + 2) & 3) * ZPL + a_lane};
      const char* const pln[3] = {smem + ((3 * c + 3) & 3) * ZPL + a_lane,
                                  smem + ((3 * c + 4) & 3) * ZPL + a_lane,
                                  smem + ((3 * c + 5) & 3) * ZPL + a_lane};
      auto stage = [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        constexpr int KZ = R / 3 - 1, KY = R % 3 - 1;
        constexpr int KZN = R < 8 ? (R + 1) / 3 - 1 : -1, KYN = R < 8 ? (R + 1) % 3 - 1 : -1;
        const int s = 9 * c + R;
        int boff = C::RING_OFF + (int)((unsigned)s % NSTL) * C::BSLOT;   // (s >= 0: no
        int bnof = C::RING_OFF + (int)((unsigned)(s + 1) % NSTL) * C::BSLOT;  // signed fixup)
        asm volatile("" : "+s"(boff), "+s"(bnof));  // per-stage bases stay opaque
        const char* bsl = smem + boff + b_lane;
        const char* bsn = smem + bnof + b_lane;
        const char* const (&plx)[3] = R < 8 ? pl : pln;
        read_b<TN, 0>(bsl, b1);
        [&]<int... F>(std::integer_sequence<int, F...>) {
          ((mma_a<TN, WM, P, KZ, KY, -1, F>(acc, a, b0), read_a<WM, P, KZ, KY, 0, F>(pl, a),
            ZP_PIN()), ...);
        }(std::make_integer_sequence<int, NF>{});
        read_b<TN, 1>(bsl, b0);
        [&]<int... F>(std::integer_sequence<int, F...>) {
          ((mma_a<TN, WM, P, KZ, KY, 0, F>(acc, a, b1), read_a<WM, P, KZ, KY, 1, F>(pl, a),
            ZP_PIN()), ...);
        }(std::make_integer_sequence<int, NF>{});
        // barrier of stage s: the weights of stage s + 1 (issued in group s + 1 - NSTL, or in
        // the prologue); younger are the groups of the NSTL - 2 stages before s
        {
          constexpr int YF = zp_younger(P, R, MORE, true, C::WI, PI);
          constexpr int YO = zp_younger(P, R, MORE, false, C::WI, PI);
          if constexpr (ZP_SKEL >= 3) {
          } else if constexpr (YF == YO) {
            wait_vm_lgkm0<YO>();
          } else {
            if (c == 0) wait_vm_lgkm0<YF>();
            else wait_vm_lgkm0<YO>();
          }
        }
        if constexpr (ZP_SKEL < 3) raw_barrier();
        auto dma = [&]() {
          if constexpr (P == 0) {
            if constexpr (R == 0) {
              issue_plane(c, 2);
              if constexpr (MORE) issue_plane(c + 1, 0);
            } else if constexpr (R == 6 && MORE) {
              issue_plane(c + 1, 1);
            }
          } else {
            if constexpr ((R == 0 || R == 3 || R == 6) && MORE) issue_plane(c + 1, R / 3);
          }
          if constexpr (MORE || R + NSTL < 9) {
            constexpr int RN = R + NSTL;             // stage s + NSTL = 9 (c + RN / 9) + RN % 9
            issue_stage_b(c + RN / 9, RN % 9, (int)((unsigned)((9 % NSTL) * c + RN) % NSTL));
          }
        };
        read_b<TN, -1>(bsn, b1);
        [&]<int... F>(std::integer_sequence<int, F...>) {
          ((mma_a<TN, WM, P, KZ, KY, 1, F>(acc, a, b0),
            read_a<WM, P, KZN, KYN, -1, F>(plx, a), F == 1 ? dma() : void(), ZP_PIN()), ...);
        }(std::make_integer_sequence<int, NF>{});
#pragma unroll
        for (int j = 0; j < TN; ++j) b0[j] = b1[j];
      };
      stage(std::integral_constant<int, 0>{});
      stage(std::integral_constant<int, 1>{});
      stage(std::integral_constant<int, 2>{});
      stage(std::integral_constant<int, 3>{});
      stage(std::integral_constant<int, 4>{});
      stage(std::integral_constant<int, 5>{});
      stage(std::integral_constant<int, 6>{});
      stage(std::integral_constant<int, 7>{});
      stage(std::integral_constant<int, 8>{});
    };
    for (int c = 0; c + 1 < g.nchunk; ++c) chunk(c, std::true_type{});
    chunk(g.nchunk - 1, std::false_type{});
  };
  auto by_pair = [&](auto wmc) {
    if (pair == 0) run_pipe(wmc, std::integral_constant<int, 0>{});
    else run_pipe(wmc, std::integral_constant<int, 1>{});
  };
  switch (wm) {                                     // wave-uniform
    case 0: by_pair(std::integral_constant<int, 0>{}); break;
    case 1: by_pair(std::integral_constant<int, 1>{}); break;
    case 2: by_pair(std::integral_constant<int, 2>{}); break;
    default: by_pair(std::integral_constant<int, 3>{}); break;
  }
  __syncthreads();                                  // planes / ring reused by the epilogue

  // ---- epilogue: tile row = L * 256 + pos * 16 + sub; acc[L * 4 + i][j][e] is row
  // (L, pos(wm, i), sub lk * 4 + e), column wn * 16 TN + j * 16 + lr
  auto dst_vox = [&](int row) -> int64_t {
    const int l = row >> 8, pos = (row >> 4) & 15, s = row & 15;
    const int ty = pos >> 2, tx = pos & 3;
    return (((int64_t)n * E + rz + 4 * (tz0 + l)) * E + (s >> 2) + 4 * ty) * E + (s & 3) + 4 * tx;
  };
  u16* ctile = reinterpret_cast<u16*>(smem);
  float cs[TN], cq[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    cs[j] = 0.f;
    cq[j] = 0.f;
    const int col = wn * 16 * TN + j * 16 + lr;
    const float bv = bias != nullptr ? bias[n0 + col] : 0.f;
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pos = i * S + ((i + wm) & 3);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = l * PP + pos * NS + lk * 4 + e;
          const float v = acc[l * 4 + i][j][e] + bv;
          ctile[row * (C::CROW / 2) + col] = f2bf(v);
          cs[j] += v;
          cq[j] += v * v;
        }
      }
  }
  __syncthreads();
  constexpr int CPR = C::BW / 8;
  static_assert(NTHR % CPR == 0, "a thread keeps one channel vector in the store loop");
  if constexpr (BNS) {                              // dgrad + BN-backward sums
    BnSum bs;
    bs.init(g.bnsc, g.bnsh, g.bnmu, g.bnis, n0 + (tid % CPR) * 8);
#pragma unroll 4
    for (int hh = 0; hh < ROWS * CPR / NTHR; ++hh) {
      const int qd = tid + NTHR * hh;
      const int row = qd / CPR, c8 = qd % CPR;
      const int64_t o = dst_vox(row) * g.Nd + n0 + c8 * 8;
      const u32x4 v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(ctile) +
                                                      row * C::CROW + c8 * 16);
      const u32x4 yv = *reinterpret_cast<const u32x4*>(g.bny + o);
      *reinterpret_cast<u32x4*>(dst + o) = v;
      bs.add(v, yv);
    }
    __syncthreads();                                // ctile reads done: reuse it below
    bnsum_flush(bs, reinterpret_cast<float*>(smem), CPR, NTHR, g.bnparts, gid * 2 + pair, g.Nd,
                n0);
    return;
  } else {
#pragma unroll 4
  for (int hh = 0; hh < ROWS * CPR / NTHR; ++hh) {
    const int qd = tid + NTHR * hh;
    const int row = qd / CPR, c8 = qd % CPR;
    const int64_t o = dst_vox(row) * g.Nd + n0 + c8 * 8;
    u32x4 v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(ctile) +
                                              row * C::CROW + c8 * 16);
    if (g.res != nullptr || g.relu) v = epi_res_relu(v, g.res ? g.res + o : nullptr, g.relu);
    *reinterpret_cast<u32x4*>(dst + o) = v;
  }
  if (stats != nullptr) {
    float* red = reinterpret_cast<float*>(smem + ROWS * C::CROW);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      cs[j] += __shfl_xor(cs[j], 16, 64);
      cs[j] += __shfl_xor(cs[j], 32, 64);
      cq[j] += __shfl_xor(cq[j], 16, 64);
      cq[j] += __shfl_xor(cq[j], 32, 64);
    }
    if (wm > 0 && lk == 0) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = wn * 16 * TN + j * 16 + lr;
        red[(wm - 1) * 2 * C::BW + col] = cs[j];
        red[(wm - 1) * 2 * C::BW + C::BW + col] = cq[j];
      }
    }
    __syncthreads();
    if (wm == 0 && lk == 0) {
      const int mt = gid * 2 + pair;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = wn * 16 * TN + j * 16 + lr;
        float ss = cs[j], qs = cq[j];
        for (int w = 1; w < 4; ++w) {               // fixed order: deterministic
          ss += red[(w - 1) * 2 * C::BW + col];
          qs += red[(w - 1) * 2 * C::BW + C::BW + col];
        }
        stats[((int64_t)mt * 2) * g.Nd + n0 + col] = ss;
        stats[((int64_t)mt * 2 + 1) * g.Nd + n0 + col] = qs;
      }
    }
  }
  }
}

// MMAD_LATTICE_ZP: 1 (default) plane-pair kernel where it fills the CUs, 0 the one-plane
// latticeconv.hip kernel, 2 plane-pair at any size; mmad_set_kernel_variant("lattice_zp", v)
// overrides it at run time (tests compare both forms in one process)
int zp_mode() { return sw(SW_LATTICE_ZP); }

}  // namespace

namespace mmad_lattice_zp {

// the route resolver (conv.hip) checks the residue-class geometry with mmad_lattice::ok; on
// top of it this form needs d = 4 (16^3 grids, 64 classes per sample) and enough tiles to
// give every CU one
bool ok(const mmad_patch::Geo& q) {
  if (zp_mode() <= 0 || q.dd != 4 || q.Cs % KC || q.Nd % 64) return false;
  if (q.Ds != 16 || q.Hs != 16 || q.Ws != 16 || q.Dd != 16 || q.Hd != 16 || q.Wd != 16)
    return false;                                   // 16^3 grids only (full 4^3 sub-lattices)
  if (q.Cs / KC < 2) return false;
  return (int64_t)q.nb * 8 * (q.Nd / 64) >= 256 || zp_mode() == 2;
}

static bool wide(const mmad_patch::Geo& q) {
  return q.Nd % 128 == 0 && (int64_t)q.nb * 8 * (q.Nd / 128) >= 256;
}

int64_t tiles(const mmad_patch::Geo& q) { return (int64_t)q.nb * 8; }

int fwd(const mmad_patch::Geo& q, const void* src, const void* wp, const float* bias, void* dst,
        float* stats, void* stream) {
  auto lds_attr = [](const void* k, int lds) {
    return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
  };
  static const bool attr = lds_attr((const void*)lattice_zp_kernel<4, false>, ZC<4>::LDS) &&
                           lds_attr((const void*)lattice_zp_kernel<2, false>, ZC<2>::LDS) &&
                           lds_attr((const void*)lattice_zp_kernel<4, true>, ZC<4>::LDS) &&
                           lds_attr((const void*)lattice_zp_kernel<2, true>, ZC<2>::LDS);
  if (!attr) return MMAD_EUNSUPPORTED;
  const bool w = wide(q);
  ZG g{};
  g.Cs = q.Cs; g.Nd = q.Nd; g.Kpad = q.Kpad;
  g.nchunk = q.Cs / KC;
  g.nbn = q.Nd / (w ? 128 : 64);
  g.res = reinterpret_cast<const u16*>(q.res);
  g.relu = q.relu;
  g.bny = reinterpret_cast<const u16*>(q.bny);
  g.bnsc = q.bnsc; g.bnsh = q.bnsh; g.bnmu = q.bnmu; g.bnis = q.bnis;
  g.bnparts = q.bnparts;
  if (g.bny != nullptr && (stats != nullptr || g.res != nullptr || g.relu || bias != nullptr))
    return MMAD_EUNSUPPORTED;                       // (one epilogue at a time)
  const int64_t nblk = mmad_lattice_zp::tiles(q) * g.nbn;
  g.xcd2 = sw(SW_ZP_XCD2) && g.nbn == 4 && (nblk / 4) % 4 == 0 && nblk % 8 == 0 ? 1 : 0;
  auto go = [&](auto kern, int lds) {
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(NTHR), lds, as_stream(stream), g,
                       (const u16*)src, (const u16*)wp, bias, (u16*)dst, stats);
  };
  const bool bns = g.bny != nullptr;
  if (w) {
    if (bns) go(lattice_zp_kernel<4, true>, ZC<4>::LDS);
    else go(lattice_zp_kernel<4, false>, ZC<4>::LDS);
  } else {
    if (bns) go(lattice_zp_kernel<2, true>, ZC<2>::LDS);
    else go(lattice_zp_kernel<2, false>, ZC<2>::LDS);
  }
  return launch_status();
}

}  // namespace mmad_lattice_zp
