// Input gradient of the MedicalNet stem (Cin 1 -> 64, 7^3, stride 2, pad 3) on MFMA, gfx950.
//
// No reference counterpart: this is autograd's gradient w.r.t. the input of conv1
// (pkg/models/mri_models/anat_cnn.py:29-31), which the reference never asks for but every
// attribution method (saliency, gradient x input, integrated gradients) needs.
//
// Residue-class form.  With stride 2 the voxels of dX fall into 8 parity classes
// p = (pz, py, px); the class value at cell (zc, yc, xc) -- voxel (2zc+pz, 2yc+py, 2xc+px) --
// is a stride-1 4x4x4 correlation of dY over zo = zc-1+jz, yo = yc-1+jy, xo = xc-1+jx with
// the tap k = 5 - 2j + p per axis (zero where k is outside [0, 6]; dY outside its grid reads
// as zero).
//
// The kernel runs it as a scatter GEMM so that the small class count does not leave MFMA
// columns empty:  P[(p, jx)][xv] = sum_{jz, jy, c} Wimg[jz][jy][(p, jx)][c] * dY[z][y][xv][c]
// is a 32 x 32 x 1024 product per output cell row and 32 dY columns (mfma_f32_32x32x16_bf16,
// A = the tap image, B = dY straight from global memory in its NDHWC layout, 16 bytes per
// lane), and dX[p][xc] = sum_jx P[(p, jx)][xc - 1 + jx] is a shifted 4-term sum taken through
// a per-wave LDS tile.  Every product of the 32 rows is a real tap except the 169 of 512
// class taps that fall outside the 7-wide kernel (zeros in the image).
//
// Work item = (sample, zc, 16 cell rows, 64-column chunk of dY); a wave owns 4 consecutive
// cell rows and both 32-column halves: each dY row it loads (8 fragments) feeds up to 4 cell
// rows, each tap fragment it reads from LDS feeds 8 MFMAs.  Chunks advance by 61 columns (a
// cell's window needs 3 neighbours).  Blocks are persistent: the 64 KiB bf16 tap image is
// copied into LDS once per block.  LDS: 64 KiB image + 4 x 8.5 KiB fp32 exchange tiles = 98 KiB.
//
// The epilogue is the pixel-shuffle store: lanes walk x = 2xc + px contiguously, so each
// (pz, py) row of the dense (n, 1, D, H, W) volume is written once with coalesced fp32 / f64
// stores, bounded by the real extents (odd D/H/W: the odd classes are one cell shorter).
// fp32 accumulation in a fixed order, no atomics: two launches are bit-identical.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int IMG_ELEMS = 4 * 4 * 4 * 64 * 8;   // [jz][jy][kk][lane][8] bf16 = 64 KiB
constexpr int ROWS = 4;                         // cell rows per wave
constexpr int YG = 4 * ROWS;                    // cell rows per work item
constexpr int XT = 64;                          // dY columns per chunk
constexpr int XSTEP = XT - 3;                   // complete cells per chunk
constexpr int SPAD = XT + 4;                    // exchange tile row stride (floats)
constexpr int LDS_BYTES = IMG_ELEMS * 2 + 4 * 32 * SPAD * 4;
constexpr int NTHR = 256;

// Tap image in MFMA A-fragment order: element e of lane l at step (jz, jy, kk) is
// A[row = l & 31][k = 8 (l >> 5) + e], row = p * 4 + jx, channel = 16 kk + k.
__global__ void stem_dgrad_pack_kernel(const float* __restrict__ w, u16* __restrict__ img) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= IMG_ELEMS) return;
  const int e = idx & 7, row = (idx >> 3) & 31, kg = (idx >> 8) & 1, kk = (idx >> 9) & 3;
  const int jy = (idx >> 11) & 3, jz = (idx >> 13) & 3;
  const int p = row >> 2, jx = row & 3;
  const int kz = 5 - 2 * jz + (p >> 2), ky = 5 - 2 * jy + ((p >> 1) & 1), kx = 5 - 2 * jx + (p & 1);
  const int c = kk * 16 + kg * 8 + e;
  float v = 0.f;
  if (kz >= 0 && kz < 7 && ky >= 0 && ky < 7 && kx >= 0 && kx < 7)
    v = w[c * 343 + kz * 49 + ky * 7 + kx];
  img[idx] = f2bf(v);
}

struct SD {
  int n, D, H, W, Do, Ho, Wo, ygroups, xchunks;
  int64_t items;
};

template <typename TO>
__global__ __launch_bounds__(NTHR) void stem_dgrad_kernel(SD g, const u16* __restrict__ dy,
                                                          const u16* __restrict__ img,
                                                          TO* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u16* simg = reinterpret_cast<u16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* S = reinterpret_cast<float*>(smem + IMG_ELEMS * 2) + wv * 32 * SPAD;
  for (int i = tid; i < IMG_ELEMS / 8; i += NTHR)
    reinterpret_cast<u32x4*>(simg)[i] = reinterpret_cast<const u32x4*>(img)[i];
  __syncthreads();
  const int col = lane & 31, half = lane >> 5;

  for (int64_t item = blockIdx.x; item < g.items; item += gridDim.x) {
    int64_t t = item;
    const int xch = (int)(t % g.xchunks); t /= g.xchunks;
    const int yg = (int)(t % g.ygroups); t /= g.ygroups;
    const int zc = (int)(t % g.Do);
    const int nb = (int)(t / g.Do);
    const int yc0 = yg * YG + wv * ROWS;
    if (yc0 >= g.Ho) continue;                      // per-wave: nothing below is block-wide
    const int s = xch * XSTEP;                      // first dY column of the chunk
    const int lo = xch == 0 ? 0 : s + 1;            // cells [lo, hi] complete in this chunk
    const int hi = s + XT - 1 >= g.Wo - 1 ? g.Wo - 1 : s + XSTEP;

    f32x16 acc[ROWS][2];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[r][nt][v] = 0.f;

    for (int jz = 0; jz < 4; ++jz) {
      const int z = zc - 1 + jz;
      if (z < 0 || z >= g.Do) continue;
      bf16x8 a[4][4];
#pragma unroll
      for (int jy = 0; jy < 4; ++jy)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          a[jy][kk] = *reinterpret_cast<const bf16x8*>(
              simg + ((((jz * 4 + jy) * 4 + kk) * 64 + lane) << 3));
      const int64_t plane = ((int64_t)nb * g.Do + z) * g.Ho;
#pragma unroll
      for (int tr = 0; tr < ROWS + 3; ++tr) {
        const int y = yc0 - 1 + tr;
        const bool rowok = y >= 0 && y < g.Ho;
        bf16x8 b[2][4];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const int xv = s + nt * 32 + col;
          const bool ok = rowok && xv < g.Wo;
          const u16* src = dy + (((plane + y) * g.Wo + xv) << 6) + half * 8;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            u32x4 q = u32x4{0u, 0u, 0u, 0u};
            if (ok) q = *reinterpret_cast<const u32x4*>(src + kk * 16);
            b[nt][kk] = __builtin_bit_cast(bf16x8, q);
          }
        }
#pragma unroll
        for (int jy = 0; jy < 4; ++jy) {
          const int r = tr - jy;                    // cell row yc0 + r reads dY row yc0+r-1+jy
          if (r < 0 || r >= ROWS) continue;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
              acc[r][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[jy][kk], b[nt][kk],
                                                                   acc[r][nt], 0, 0, 0);
        }
      }
    }

    // dX[p][xc] = sum_jx P[p*4 + jx][xc - 1 + jx], one cell row at a time through the wave's
    // own LDS tile (LDS ops of one wave complete in order; the waits order them for the
    // compiler too)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int yc = yc0 + r;
      if (yc >= g.Ho) break;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          S[((v & 3) + 8 * (v >> 2) + 4 * half) * SPAD + nt * 32 + col] = acc[r][nt][v];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const int xend = min(2 * hi + 1, g.W - 1);
      for (int q = 0; q < 4; ++q) {
        const int z = 2 * zc + (q >> 1), y = 2 * yc + (q & 1);
        if (z >= g.D || y >= g.H) continue;
        TO* drow = dx + (((int64_t)nb * g.D + z) * g.H + y) * g.W;
        for (int x = 2 * lo + lane; x <= xend; x += 64) {
          const int p = q * 2 + (x & 1);
          const int c0 = (x >> 1) - 1 - s;
          float sum = 0.f;
#pragma unroll
          for (int jx = 0; jx < 4; ++jx) {
            const int c = c0 + jx;
            if (c >= 0 && c < XT) sum += S[(p * 4 + jx) * SPAD + c];
          }
          drow[x] = (TO)sum;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int xchunks_of(int wo) {
  int c = 1;
  for (int s = 0; s + XT - 1 < wo - 1; s += XSTEP) ++c;
  return c;
}

}  // namespace

extern "C" {

int mmad_stem_dgrad_ok(const mmad_conv_desc* d, int dtype, int out_dtype) {
  if (!d || dtype != MMAD_BF16 || (out_dtype != MMAD_F32 && out_dtype != MMAD_F64)) return 0;
  if (d->n <= 0 || d->di <= 0 || d->hi <= 0 || d->wi <= 0) return 0;
  if (d->ci != 1 || d->co != 64) return 0;
  if (d->kd != 7 || d->kh != 7 || d->kw != 7 || d->sd != 2 || d->sh != 2 || d->sw != 2) return 0;
  if (d->pd != 3 || d->ph != 3 || d->pw != 3 || d->dd != 1 || d->dh != 1 || d->dw != 1) return 0;
  if (d->do_ != (d->di + 1) / 2 || d->ho != (d->hi + 1) / 2 || d->wo != (d->wi + 1) / 2) return 0;
  // the x coordinate and the per-row offsets are 32-bit; everything else is 64-bit
  return d->wi < (1 << 28) ? 1 : 0;
}

int64_t mmad_stem_dgrad_ws_bytes(const mmad_conv_desc* d) {
  (void)d;
  return (int64_t)IMG_ELEMS * 2;
}

int mmad_conv3d_dgrad_raw(const mmad_conv_desc* d, int dtype, const void* dy, const float* w,
                          int out_dtype, void* dx, void* ws, void* stream) {
  if (!d) return MMAD_ENULL;
  if (d->n <= 0 || d->di <= 0 || d->hi <= 0 || d->wi <= 0 || d->ci <= 0 || d->co <= 0)
    return MMAD_EBADSHAPE;
  if (dtype != MMAD_F32 && dtype != MMAD_BF16) return MMAD_EBADDTYPE;
  if (out_dtype != MMAD_F32 && out_dtype != MMAD_F64) return MMAD_EBADDTYPE;
  if (!dy || !w || !dx || !ws) return MMAD_ENULL;
  if (!aligned16(dy) || !aligned16(w) || !aligned16(dx) || !aligned16(ws)) return MMAD_EBADSHAPE;
  if (!mmad_stem_dgrad_ok(d, dtype, out_dtype)) return MMAD_EUNSUPPORTED;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(stem_dgrad_pack_kernel, dim3(IMG_ELEMS / 256), dim3(256), 0, st, w,
                     (u16*)ws);
  int rc = launch_status();
  if (rc) return rc;
  SD g{};
  g.n = d->n; g.D = d->di; g.H = d->hi; g.W = d->wi;
  g.Do = d->do_; g.Ho = d->ho; g.Wo = d->wo;
  g.ygroups = (int)cdiv(d->ho, YG);
  g.xchunks = xchunks_of(d->wo);
  g.items = (int64_t)d->n * d->do_ * g.ygroups * g.xchunks;
  const unsigned grid = (unsigned)std::min<int64_t>(g.items, 256);   // one block per CU
  if (out_dtype == MMAD_F32) {
    static const bool attr =
        hipFuncSetAttribute((const void*)stem_dgrad_kernel<float>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess;
    if (!attr) return MMAD_EUNSUPPORTED;
    hipLaunchKernelGGL(stem_dgrad_kernel<float>, dim3(grid), dim3(NTHR), LDS_BYTES, st, g,
                       (const u16*)dy, (const u16*)ws, (float*)dx);
  } else {
    static const bool attr =
        hipFuncSetAttribute((const void*)stem_dgrad_kernel<double>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess;
    if (!attr) return MMAD_EUNSUPPORTED;
    hipLaunchKernelGGL(stem_dgrad_kernel<double>, dim3(grid), dim3(NTHR), LDS_BYTES, st, g,
                       (const u16*)dy, (const u16*)ws, (double*)dx);
  }
  return launch_status();
}

}  // extern "C"
