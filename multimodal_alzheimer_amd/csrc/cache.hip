// Device-resident dataset cache, gfx950: a whole sample table's volumes kept in HBM in a
// compact but exact form, and each batch assembled on the device from an index.  Replaces the
// DataLoader's collate + .to(device) and nibabel's get_fdata widening on the loader workers
// (pkg/utils/dataloader.py:197-211); no reference counterpart as code.
//
//   store_kernel<T>       float64 scans -> storage dtype T at consecutive slots; every voxel's
//                         widened stored value is compared with its source bit for bit and the
//                         mismatches are counted (per block, then count_finish_kernel);
//   pack_mask_kernel      float64 masks -> 1 bit per voxel, one wave ballot per 64 voxels (a
//                         lane writes whole 64-bit words, nothing is read-modify-written);
//                         voxels that are neither 0.0 nor 1.0 are counted the same way;
//   count_finish_kernel   the second stage: one block sums the per-block counts in a fixed
//                         order and adds the total to the caller's counter (the only atomic);
//   fetch_flat_kernel<K>  out[b] = widen(store[order[cursor + b]]), geometry unchanged: 16-byte
//                         loads and stores, several in flight per lane, a per-element tail;
//   fetch_pad_kernel<K>   the same with centred padding / cropping per axis: one wave per output
//                         row, 16-byte stores along W, row heads and tails per element;
//   fetch_rows_kernel     labels and tabular rows by the same index.
//
// Layout: slot s of a store starts at byte s * stride, stride = the scan's bytes rounded up to
// 16, so every scan starts 16-byte aligned.  Bits: voxel v is bit v % 8 of byte v / 8.
// The index and the cursor are read on the device when the kernel runs, so a captured launch
// moves on with the cursor.  An order position or a sample index out of range is never
// dereferenced: that batch entry is written as zeros and *bad is set to 1 (a plain store).
// All per-voxel offsets are 32-bit inside one scan (vox < 2^31); the 64-bit part is the
// scan's base, computed once per batch entry or output row.
#include <algorithm>

#include "common.h"

namespace {

constexpr int MAX_PARTS = 2048;       // blocks of a counting kernel = rows of its workspace
constexpr int MAX_BLOCKS = 2048;      // 256 CUs x 8 blocks: memory-bound grids stride the rest

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

int64_t stride_bytes(int kind, int64_t vox) {
  int64_t raw;
  switch (kind) {
    case MMAD_F64: raw = vox * 8; break;
    case MMAD_F32: raw = vox * 4; break;
    case MMAD_F16: raw = vox * 2; break;
    case MMAD_BITS: raw = (vox + 7) / 8; break;
    default: return -1;
  }
  return (raw + 15) & ~int64_t(15);
}

// double -> storage -> double.  float16 narrows through float32, as torch's x.half() does.
template <typename T> __device__ __forceinline__ T narrow(double v) { return (T)v; }
template <> __device__ __forceinline__ _Float16 narrow<_Float16>(double v) {
  float f = (float)v;
  // keep the two roundings apart: left to itself hipcc narrows double -> half in one step
  // (one rounding), which differs from torch's double -> float -> half on float-level ties
  asm volatile("" : "+v"(f));
  return (_Float16)f;
}
template <typename T> __device__ __forceinline__ double widen(T s) { return (double)s; }
template <> __device__ __forceinline__ double widen<_Float16>(_Float16 s) {
  return (double)(float)s;
}
__device__ __forceinline__ uint64_t bits_of(double v) {
  return (uint64_t)__double_as_longlong(v);
}

// this block's count -> parts[blockIdx.x] (every block writes, zero included)
__device__ __forceinline__ void block_count_to_parts(uint32_t c, uint64_t* __restrict__ parts) {
  __shared__ uint32_t wsum[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) parts[blockIdx.x] = (uint64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// item = (scan, chunk of 1024 voxels): four coalesced 8-byte loads per lane, then the stores
template <typename T>
__global__ __launch_bounds__(256) void store_kernel(uint32_t items, uint32_t vox,
                                                    uint32_t chunks, int64_t stride,
                                                    const double* __restrict__ src,
                                                    char* __restrict__ store,
                                                    uint64_t* __restrict__ parts) {
  uint32_t bad = 0;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t s = item / chunks, c = item - s * chunks;
    const double* __restrict__ in = src + (int64_t)s * vox;
    T* __restrict__ dst = reinterpret_cast<T*>(store + (int64_t)s * stride);
    const uint32_t e0 = c * 1024u + threadIdx.x;
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t e = e0 + k * 256u;
      v[k] = e < vox ? in[e] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t e = e0 + k * 256u;
      if (e < vox) {
        const T t = narrow<T>(v[k]);
        dst[e] = t;
        bad += bits_of(widen<T>(t)) != bits_of(v[k]) ? 1u : 0u;
      }
    }
  }
  block_count_to_parts(bad, parts);
}

// item = (scan, chunk of 2048 voxels): each wave takes 512 of them in eight ballots
__global__ __launch_bounds__(256) void pack_mask_kernel(uint32_t items, uint32_t vox,
                                                        uint32_t chunks, int64_t stride,
                                                        const double* __restrict__ src,
                                                        char* __restrict__ store,
                                                        uint64_t* __restrict__ parts) {
  constexpr uint64_t ONE = 0x3ff0000000000000ull;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t bad = 0;                       // counted on lane 0 of each wave
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t s = item / chunks, c = item - s * chunks;
    const double* __restrict__ in = src + (int64_t)s * vox;
    uint64_t* __restrict__ dst = reinterpret_cast<uint64_t*>(store + (int64_t)s * stride);
    const uint32_t base = c * 2048u + wave * 512u;
    uint64_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t e = base + k * 64u + lane;
      v[k] = e < vox ? bits_of(in[e]) : 0;          // past the end: a zero bit, not counted
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint64_t word = __ballot(v[k] == ONE);
      const uint64_t odd = __ballot(v[k] != ONE && v[k] != 0);
      // word w covers voxels [64 w, 64 w + 64): inside the stride, which is ceil(vox / 8)
      // rounded up to 16 bytes
      if (lane == 0 && base + k * 64u < vox) {
        dst[(base + k * 64u) >> 6] = word;
        bad += (uint32_t)__popcll(odd);
      }
    }
  }
  block_count_to_parts(bad, parts);
}

__global__ __launch_bounds__(256) void count_finish_kernel(const uint64_t* __restrict__ parts,
                                                           int nparts,
                                                           unsigned long long* counter) {
  __shared__ uint64_t sums[256];
  uint64_t s = 0;
  for (int i = threadIdx.x; i < nparts; i += 256) s += parts[i];
  sums[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sums[threadIdx.x] += sums[threadIdx.x + o];
    __syncthreads();
  }
  // an integer sum: the result does not depend on the order in which launches arrive
  if (threadIdx.x == 0 && sums[0] != 0) atomicAdd(counter, (unsigned long long)sums[0]);
}

// ---- reading the store: N elements per 16-byte unit, one element, an aligned pair ------
template <int KIND> struct Src;
template <> struct Src<MMAD_F64> {
  static constexpr int N = 2;
  static __device__ __forceinline__ void unit(const char* p, uint32_t u, double* v) {
    const f64x2 c = reinterpret_cast<const f64x2*>(p)[u];
    v[0] = c[0]; v[1] = c[1];
  }
  static __device__ __forceinline__ double one(const char* p, uint32_t e) {
    return reinterpret_cast<const double*>(p)[e];
  }
  static __device__ __forceinline__ void pair(const char* p, uint32_t e, double& a, double& b) {
    const f64x2 c = reinterpret_cast<const f64x2*>(p)[e >> 1];
    a = c[0]; b = c[1];
  }
};
template <> struct Src<MMAD_F32> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void unit(const char* p, uint32_t u, double* v) {
    const f32x4 c = reinterpret_cast<const f32x4*>(p)[u];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (double)c[i];
  }
  static __device__ __forceinline__ double one(const char* p, uint32_t e) {
    return (double)reinterpret_cast<const float*>(p)[e];
  }
  static __device__ __forceinline__ void pair(const char* p, uint32_t e, double& a, double& b) {
    const f32x2 c = reinterpret_cast<const f32x2*>(p)[e >> 1];
    a = (double)c[0]; b = (double)c[1];
  }
};
template <> struct Src<MMAD_F16> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unit(const char* p, uint32_t u, double* v) {
    const f16x8 c = reinterpret_cast<const f16x8*>(p)[u];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = widen<_Float16>(c[i]);
  }
  static __device__ __forceinline__ double one(const char* p, uint32_t e) {
    return widen<_Float16>(reinterpret_cast<const _Float16*>(p)[e]);
  }
  static __device__ __forceinline__ void pair(const char* p, uint32_t e, double& a, double& b) {
    const f16x2 c = reinterpret_cast<const f16x2*>(p)[e >> 1];
    a = widen<_Float16>(c[0]); b = widen<_Float16>(c[1]);
  }
};
// bits: a unit is the two voxels of one 16-byte store; the 32-bit word is shared by 16 lanes
template <> struct Src<MMAD_BITS> {
  static constexpr int N = 2;
  static __device__ __forceinline__ double one(const char* p, uint32_t e) {
    return (reinterpret_cast<const uint32_t*>(p)[e >> 5] >> (e & 31u)) & 1u ? 1.0 : 0.0;
  }
  static __device__ __forceinline__ void pair(const char* p, uint32_t e, double& a, double& b) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(p)[e >> 5] >> (e & 31u);   // e even
    a = w & 1u ? 1.0 : 0.0; b = w & 2u ? 1.0 : 0.0;
  }
  static __device__ __forceinline__ void unit(const char* p, uint32_t u, double* v) {
    pair(p, u * 2u, v[0], v[1]);
  }
};

// the sample behind batch entry b, or -1: nothing out of range is ever dereferenced
__device__ __forceinline__ int64_t entry_index(const int64_t* __restrict__ order,
                                               int64_t cur, int64_t order_len, int64_t n,
                                               int b) {
  const int64_t pos = cur + b;
  if (pos < 0 || pos >= order_len) return -1;
  const int64_t idx = order[pos];
  return idx >= 0 && idx < n ? idx : -1;
}

template <int N>
__device__ __forceinline__ void store_unit(double* __restrict__ dst, const double* v) {
#pragma unroll
  for (int i = 0; i < N; i += 2) {
    f64x2 c; c[0] = v[i]; c[1] = v[i + 1];
    *reinterpret_cast<f64x2*>(dst + i) = c;
  }
}

// geometry unchanged: blockIdx.y = batch entry, blockIdx.x strides over the scan
template <int KIND>
__global__ __launch_bounds__(256) void fetch_flat_kernel(uint32_t vox, int64_t n, int64_t stride,
                                                         const char* __restrict__ store,
                                                         const int64_t* __restrict__ order,
                                                         const int64_t* __restrict__ cursor,
                                                         int64_t order_len,
                                                         double* __restrict__ out,
                                                         int32_t* __restrict__ bad) {
  using S = Src<KIND>;
  constexpr int N = S::N;
  const int b = blockIdx.y;
  const int64_t idx = entry_index(order, cursor ? *cursor : 0, order_len, n, b);
  double* __restrict__ dst = out + (int64_t)b * vox;
  const uint32_t tid = blockIdx.x * 256u + threadIdx.x, nth = gridDim.x * 256u;
  if (idx < 0) {
    if (tid == 0) *bad = 1;
    for (uint32_t e = tid; e < vox; e += nth) dst[e] = 0.0;
    return;
  }
  const char* __restrict__ src = store + idx * stride;
  if ((reinterpret_cast<uintptr_t>(dst) & 15u) != 0) {
    // an odd voxel count puts every other entry 8 bytes off: coalesced 8-byte stores
    for (uint32_t e = tid; e < vox; e += nth) dst[e] = S::one(src, e);
    return;
  }
  const uint32_t units = vox / N;
  uint32_t u = tid;
  for (; u + 3u * nth < units; u += 4u * nth) {         // four 16-byte loads in flight per lane
    double v[4][N];
#pragma unroll
    for (int k = 0; k < 4; ++k) S::unit(src, u + k * nth, v[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) store_unit<N>(dst + (u + k * nth) * N, v[k]);
  }
  for (; u < units; u += nth) {
    double v[N];
    S::unit(src, u, v);
    store_unit<N>(dst + u * N, v);
  }
  for (uint32_t e = units * N + tid; e < vox; e += nth) dst[e] = S::one(src, e);
}

struct Geom {
  int di, hi, wi;       // stored extent
  int dout, hout, wout; // output extent
  int od, oh, ow;       // floor((out - in) / 2): negative crops, positive zero-fills
};

// one wave per output row (b, z, y); lanes run along W in 16-byte pairs
template <int KIND>
__global__ __launch_bounds__(256) void fetch_pad_kernel(Geom g, uint32_t rows, int64_t n,
                                                        int64_t stride,
                                                        const char* __restrict__ store,
                                                        const int64_t* __restrict__ order,
                                                        const int64_t* __restrict__ cursor,
                                                        int64_t order_len,
                                                        double* __restrict__ out,
                                                        int32_t* __restrict__ bad) {
  using S = Src<KIND>;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * 4u;
  const int64_t cur = cursor ? *cursor : 0;
  for (uint32_t r = wave; r < rows; r += nwaves) {
    const uint32_t plane = r / (uint32_t)g.hout, y = r - plane * (uint32_t)g.hout;
    const uint32_t b = plane / (uint32_t)g.dout, z = plane - b * (uint32_t)g.dout;
    const int64_t idx = entry_index(order, cur, order_len, n, (int)b);
    if (idx < 0 && lane == 0) *bad = 1;
    const int zi = (int)z - g.od, yi = (int)y - g.oh;
    const bool inside = idx >= 0 && (unsigned)zi < (unsigned)g.di && (unsigned)yi < (unsigned)g.hi;
    const char* __restrict__ src = store + (inside ? idx : 0) * stride;
    const int srow = inside ? (zi * g.hi + yi) * g.wi : 0;       // < vox < 2^31
    double* __restrict__ drow = out + (int64_t)r * g.wout;
    auto elem = [&](int x) -> double {
      const int xi = x - g.ow;
      return inside && (unsigned)xi < (unsigned)g.wi ? S::one(src, (uint32_t)(srow + xi)) : 0.0;
    };
    // h: elements before the row's first 16-byte boundary (an odd W' alternates it)
    const int h = (int)((reinterpret_cast<uintptr_t>(drow) >> 3) & 1u);
    const int npair = (g.wout - h) >> 1;
    const bool src_even = ((srow + h - g.ow) & 1) == 0;
    for (int p = lane; p < npair; p += 64) {
      const int x = h + 2 * p, xi = x - g.ow;
      f64x2 c;
      if (inside && src_even && xi >= 0 && xi + 1 < g.wi) {
        double a, bb;
        S::pair(src, (uint32_t)(srow + xi), a, bb);
        c[0] = a; c[1] = bb;
      } else {
        c[0] = elem(x); c[1] = elem(x + 1);
      }
      *reinterpret_cast<f64x2*>(drow + x) = c;
    }
    if (lane == 0 && h) drow[0] = elem(0);
    if (lane == 1 && ((g.wout - h) & 1)) drow[g.wout - 1] = elem(g.wout - 1);
  }
}

__global__ __launch_bounds__(256) void fetch_rows_kernel(int nb, int cols, int64_t n,
                                                         const int64_t* __restrict__ labels,
                                                         const double* __restrict__ tab,
                                                         const int64_t* __restrict__ order,
                                                         const int64_t* __restrict__ cursor,
                                                         int64_t order_len,
                                                         int64_t* __restrict__ out_labels,
                                                         double* __restrict__ out_tab,
                                                         int32_t* __restrict__ bad) {
  const int64_t cur = cursor ? *cursor : 0;
  const int per = cols + 1;                           // column `cols` is the label
  for (int t = threadIdx.x; t < nb * per; t += 256) {
    const int b = t / per, c = t - b * per;
    const int64_t idx = entry_index(order, cur, order_len, n, b);
    if (idx < 0) *bad = 1;
    if (c == cols) {
      if (out_labels) out_labels[b] = idx < 0 ? 0 : labels[idx];
    } else if (out_tab) {
      out_tab[(int64_t)b * cols + c] = idx < 0 ? 0.0 : tab[idx * cols + c];
    }
  }
}

bool value_kind(int kind) { return kind == MMAD_F64 || kind == MMAD_F32 || kind == MMAD_F16; }

// shared argument checks of the two fill entries; returns MMAD_OK and the launch shape
int fill_args(int n, int64_t vox, const void* src, const void* store, int64_t slot0,
              int64_t capacity, const void* counter, const void* ws, uint32_t per_chunk,
              uint32_t* chunks, uint32_t* items) {
  if (n <= 0 || vox <= 0 || slot0 < 0 || capacity <= 0 || slot0 > capacity - n)
    return MMAD_EBADSHAPE;
  if (vox >= (int64_t(1) << 31)) return MMAD_EUNSUPPORTED;
  if (!src || !store || !counter || !ws) return MMAD_ENULL;
  if ((reinterpret_cast<uintptr_t>(store) & 15u) || (reinterpret_cast<uintptr_t>(src) & 7u) ||
      (reinterpret_cast<uintptr_t>(ws) & 7u) || (reinterpret_cast<uintptr_t>(counter) & 7u))
    return MMAD_EBADSHAPE;
  const int64_t c = cdiv(vox, per_chunk), it = c * n;
  if (it >= (int64_t(1) << 31)) return MMAD_EUNSUPPORTED;
  *chunks = (uint32_t)c;
  *items = (uint32_t)it;
  return MMAD_OK;
}

}  // namespace

extern "C" {

int64_t mmad_cache_stride_bytes(int kind, int64_t vox) {
  return vox > 0 ? stride_bytes(kind, vox) : -1;
}

int64_t mmad_cache_ws_bytes(void) { return (int64_t)MAX_PARTS * 8; }

int mmad_cache_store(int kind, int n, int64_t vox, const double* src, void* store, int64_t slot0,
                     int64_t capacity, uint64_t* mismatches, void* ws, void* stream) {
  if (!value_kind(kind)) return MMAD_EBADDTYPE;
  uint32_t chunks, items;
  const int rc = fill_args(n, vox, src, store, slot0, capacity, mismatches, ws, 1024u, &chunks,
                           &items);
  if (rc != MMAD_OK) return rc;
  const int64_t stride = stride_bytes(kind, vox);
  char* base = static_cast<char*>(store) + slot0 * stride;
  const unsigned grid = (unsigned)std::min<uint32_t>(items, MAX_PARTS);
  uint64_t* parts = static_cast<uint64_t*>(ws);
  hipStream_t st = as_stream(stream);
  if (kind == MMAD_F64)
    hipLaunchKernelGGL(store_kernel<double>, dim3(grid), dim3(256), 0, st, items, (uint32_t)vox,
                       chunks, stride, src, base, parts);
  else if (kind == MMAD_F32)
    hipLaunchKernelGGL(store_kernel<float>, dim3(grid), dim3(256), 0, st, items, (uint32_t)vox,
                       chunks, stride, src, base, parts);
  else
    hipLaunchKernelGGL(store_kernel<_Float16>, dim3(grid), dim3(256), 0, st, items,
                       (uint32_t)vox, chunks, stride, src, base, parts);
  hipLaunchKernelGGL(count_finish_kernel, dim3(1), dim3(256), 0, st, parts, (int)grid,
                     reinterpret_cast<unsigned long long*>(mismatches));
  return launch_status();
}

int mmad_cache_pack_mask(int n, int64_t vox, const double* src, void* store, int64_t slot0,
                         int64_t capacity, uint64_t* nonbinary, void* ws, void* stream) {
  uint32_t chunks, items;
  const int rc = fill_args(n, vox, src, store, slot0, capacity, nonbinary, ws, 2048u, &chunks,
                           &items);
  if (rc != MMAD_OK) return rc;
  const int64_t stride = stride_bytes(MMAD_BITS, vox);
  char* base = static_cast<char*>(store) + slot0 * stride;
  const unsigned grid = (unsigned)std::min<uint32_t>(items, MAX_PARTS);
  uint64_t* parts = static_cast<uint64_t*>(ws);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(pack_mask_kernel, dim3(grid), dim3(256), 0, st, items, (uint32_t)vox, chunks,
                     stride, src, base, parts);
  hipLaunchKernelGGL(count_finish_kernel, dim3(1), dim3(256), 0, st, parts, (int)grid,
                     reinterpret_cast<unsigned long long*>(nonbinary));
  return launch_status();
}

int mmad_cache_fetch(int kind, int b, int64_t n, int di, int hi, int wi, int dout, int hout,
                     int wout, const void* store, const int64_t* order, const int64_t* cursor,
                     int64_t order_len, double* out, int32_t* bad, void* stream) {
  if (!value_kind(kind) && kind != MMAD_BITS) return MMAD_EBADDTYPE;
  if (b <= 0 || b > 65535 || n <= 0 || order_len <= 0 || di <= 0 || hi <= 0 || wi <= 0 ||
      dout <= 0 || hout <= 0 || wout <= 0)
    return MMAD_EBADSHAPE;
  const int64_t vox = (int64_t)di * hi * wi, vout = (int64_t)dout * hout * wout;
  const int64_t rows = (int64_t)b * dout * hout;
  if (vox >= (int64_t(1) << 31) || vout >= (int64_t(1) << 31) || rows >= (int64_t(1) << 31))
    return MMAD_EUNSUPPORTED;
  if (!store || !order || !out || !bad) return MMAD_ENULL;
  if ((reinterpret_cast<uintptr_t>(store) & 15u) || (reinterpret_cast<uintptr_t>(out) & 7u) ||
      (reinterpret_cast<uintptr_t>(order) & 7u) || (reinterpret_cast<uintptr_t>(cursor) & 7u) ||
      (reinterpret_cast<uintptr_t>(bad) & 3u))
    return MMAD_EBADSHAPE;
  const int64_t stride = stride_bytes(kind, vox);
  const char* base = static_cast<const char*>(store);
  hipStream_t st = as_stream(stream);
#define MMAD_CACHE_BY_KIND(LAUNCH)                      \
  switch (kind) {                                       \
    case MMAD_F64: LAUNCH(MMAD_F64); break;             \
    case MMAD_F32: LAUNCH(MMAD_F32); break;             \
    case MMAD_F16: LAUNCH(MMAD_F16); break;             \
    default: LAUNCH(MMAD_BITS); break;                  \
  }
  if (di == dout && hi == hout && wi == wout) {
    // about MAX_BLOCKS blocks in all, and no more than the scan has 16-byte units for
    const int64_t want = cdiv(MAX_BLOCKS, b), have = cdiv(cdiv(vox, 2), 256);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min(want, have)), (unsigned)b);
#define MMAD_CACHE_FLAT(K)                                                                     \
  hipLaunchKernelGGL(fetch_flat_kernel<K>, grid, dim3(256), 0, st, (uint32_t)vox, n, stride,   \
                     base, order, cursor, order_len, out, bad)
    MMAD_CACHE_BY_KIND(MMAD_CACHE_FLAT)
#undef MMAD_CACHE_FLAT
  } else {
    auto off = [](int o, int i) { return (o - i) >= 0 ? (o - i) / 2 : -((i - o + 1) / 2); };
    const Geom g{di, hi, wi, dout, hout, wout, off(dout, di), off(hout, hi), off(wout, wi)};
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(rows, 4), MAX_BLOCKS));
#define MMAD_CACHE_PAD(K)                                                                      \
  hipLaunchKernelGGL(fetch_pad_kernel<K>, grid, dim3(256), 0, st, g, (uint32_t)rows, n, stride, \
                     base, order, cursor, order_len, out, bad)
    MMAD_CACHE_BY_KIND(MMAD_CACHE_PAD)
#undef MMAD_CACHE_PAD
  }
#undef MMAD_CACHE_BY_KIND
  return launch_status();
}

int mmad_cache_fetch_rows(int b, int64_t n, int cols, const int64_t* labels, const double* tab,
                          const int64_t* order, const int64_t* cursor, int64_t order_len,
                          int64_t* out_labels, double* out_tab, int32_t* bad, void* stream) {
  if (b <= 0 || b > 65535 || n <= 0 || order_len <= 0 || cols < 0 || cols > 4096)
    return MMAD_EBADSHAPE;
  if (!order || !bad || (out_labels && !labels) || (out_tab && !tab)) return MMAD_ENULL;
  if (!out_labels && !out_tab) return MMAD_ENULL;
  if (out_tab && cols == 0) return MMAD_EBADSHAPE;
  hipLaunchKernelGGL(fetch_rows_kernel, dim3(1), dim3(256), 0, as_stream(stream), b, cols, n,
                     labels, tab, order, cursor, order_len, out_labels, out_tab, bad);
  return launch_status();
}

}  // extern "C"
