// Occlusion sensitivity, gfx950: the three small kernels around a captured eval forward
// (explain.occlusion).  No reference counterpart: the reference has no attribution code.
//
//   occlude_kernel<T, N>  moves the occluding windows of m * b forward rows by one replay: the
//                         new window of each slot is filled, what the previous replay filled and
//                         the new window does not cover is restored from the source.  Both sets
//                         follow from (source, cursor) alone and are disjoint, so no thread
//                         depends on another.  Lanes run along W; N elements per 16-byte unit
//                         where every row start allows it (N = 1: the element path);
//   drop_kernel           base score - score of each forward row -> the drops table at the rows
//                         the cursor names;
//   map_kernel            drops -> per-voxel mean over the covering windows: a gather in
//                         ascending window order, float64, one rounding, no atomics.
//
// The window rule is restated from explain.occlusion_windows (include/mmad.h): per axis
// n = max(1, ceil((s - p) / t) + 1) windows start at min(i * t, s - p).
// The cursor is read on the device when the kernel runs, so a captured launch moves on with it;
// a window index outside [0, nwin) selects nothing.  All per-voxel offsets are 32-bit inside one
// volume (vox < 2^31); the 64-bit part is the volume's base.
#include <algorithm>

#include "common.h"

// the map's sum and quotient are the stated operations, one by one (no fused multiply-add)
#pragma clang fp contract(off)

namespace {

constexpr int MAX_BLOCKS = 2048;
constexpr int MODE_LOGIT = 0, MODE_PROB = 1;

typedef double f64x2 __attribute__((ext_vector_type(2)));

struct Geo {
  int d, h, w;        // volume extent
  int pd, ph, pw;     // patch
  int td, th, tw;     // stride
  int nd, nh, nw;     // windows per axis
};

inline int axis_windows(int s, int p, int t) { return std::max(1, (int)cdiv(s - p, t) + 1); }

// shared argument checks; fills the per-axis window counts
int geo_args(int d, int h, int w, int pd, int ph, int pw, int td, int th, int tw, int64_t nwin,
             Geo* g) {
  if (d <= 0 || h <= 0 || w <= 0 || pd < 1 || ph < 1 || pw < 1 || pd > d || ph > h || pw > w ||
      td < 1 || th < 1 || tw < 1 || td > pd || th > ph || tw > pw)
    return MMAD_EBADSHAPE;
  if ((int64_t)d * h * w >= (int64_t(1) << 31)) return MMAD_EUNSUPPORTED;
  *g = Geo{d, h, w, pd, ph, pw, td, th, tw, axis_windows(d, pd, td), axis_windows(h, ph, th),
           axis_windows(w, pw, tw)};
  if (nwin != (int64_t)g->nd * g->nh * g->nw) return MMAD_EBADSHAPE;
  return MMAD_OK;
}

struct Win { int z, y, x; };

// the corner of window j, 0 <= j < nwin
__device__ __forceinline__ Win window_of(const Geo& g, int64_t j) {
  const int ix = (int)(j % g.nw);
  const int64_t r = j / g.nw;
  const int iy = (int)(r % g.nh), iz = (int)(r / g.nh);
  return Win{min(iz * g.td, g.d - g.pd), min(iy * g.th, g.h - g.ph), min(ix * g.tw, g.w - g.pw)};
}

__device__ __forceinline__ bool in_window(const Geo& g, const Win& wn, int z, int y, int x) {
  return (unsigned)(z - wn.z) < (unsigned)g.pd && (unsigned)(y - wn.y) < (unsigned)g.ph &&
         (unsigned)(x - wn.x) < (unsigned)g.pw;
}

template <typename T, int N> struct Unit;
template <typename T> struct Unit<T, 1> {
  static __device__ __forceinline__ void copy(T* dst, const T* src) { *dst = *src; }
  static __device__ __forceinline__ void set(T* dst, T v) { *dst = v; }
};
template <> struct Unit<double, 2> {
  static __device__ __forceinline__ void copy(double* dst, const double* src) {
    *reinterpret_cast<f64x2*>(dst) = *reinterpret_cast<const f64x2*>(src);
  }
  static __device__ __forceinline__ void set(double* dst, double v) {
    f64x2 c; c[0] = v; c[1] = v;
    *reinterpret_cast<f64x2*>(dst) = c;
  }
};
template <> struct Unit<float, 4> {
  static __device__ __forceinline__ void copy(float* dst, const float* src) {
    *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(src);
  }
  static __device__ __forceinline__ void set(float* dst, float v) {
    f32x4 c; c[0] = v; c[1] = v; c[2] = v; c[3] = v;
    *reinterpret_cast<f32x4*>(dst) = c;
  }
};

// the items of one slot: (which, row, unit), unit fastest; which 0 = the new window (fill),
// 1 = the old one (restore where the new one does not cover).  With N > 1 both windows' x
// offsets, w and pw are multiples of N, so a unit lies wholly inside or outside a window.
template <typename T, int N>
__device__ __forceinline__ void move_windows(const Geo& g, bool has_new, bool has_old,
                                             const Win& wn, const Win& wo, T f,
                                             const T* __restrict__ s, T* __restrict__ dst) {
  const int upr = g.pw / N, per = g.pd * g.ph * upr;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < 2 * per; t += gridDim.x * 256) {
    const int which = t >= per, q = t - which * per;
    const int row = q / upr, u = q - row * upr;
    const int rz = row / g.ph, ry = row - rz * g.ph;
    if (which == 0) {
      if (!has_new) continue;
      const int e = ((wn.z + rz) * g.h + wn.y + ry) * g.w + wn.x + u * N;    // < vox < 2^31
      Unit<T, N>::set(dst + e, f);
    } else {
      if (!has_old) continue;
      const int z = wo.z + rz, y = wo.y + ry, x = wo.x + u * N;
      if (has_new && in_window(g, wn, z, y, x)) continue;
      const int e = (z * g.h + y) * g.w + x;
      Unit<T, N>::copy(dst + e, s + e);
    }
  }
}

// blockIdx.y = slot, blockIdx.x strides over the slot's items
template <typename T, int N>
__global__ __launch_bounds__(256) void occlude_kernel(Geo g, int b, int m, int64_t nwin,
                                                      int vec_ok, const T* __restrict__ src,
                                                      T* __restrict__ slots,
                                                      const double* __restrict__ fill,
                                                      const int64_t* __restrict__ cursor) {
  const int slot = blockIdx.y, sample = slot % b, k = slot / b;
  const int64_t cur = *cursor;
  const int64_t jn = cur + k, jo = cur - m + k;
  const bool has_new = jn >= 0 && jn < nwin, has_old = jo >= 0 && jo < nwin;
  if (!has_new && !has_old) return;
  const Win wn = window_of(g, has_new ? jn : 0), wo = window_of(g, has_old ? jo : 0);
  const int64_t vox = (int64_t)g.d * g.h * g.w;
  const T* __restrict__ s = src + sample * vox;
  T* __restrict__ dst = slots + slot * vox;
  const T f = (T)fill[sample];
  // slot-uniform: every row of both windows starts on a 16-byte boundary
  const bool vec = N > 1 && vec_ok && (!has_new || wn.x % N == 0) && (!has_old || wo.x % N == 0);
  if (vec) move_windows<T, N>(g, has_new, has_old, wn, wo, f, s, dst);
  else move_windows<T, 1>(g, has_new, has_old, wn, wo, f, s, dst);
}

__global__ __launch_bounds__(256) void drop_kernel(int mode, int b, int m, int c, int64_t nwin,
                                                   const double* __restrict__ logits,
                                                   const int64_t* __restrict__ target,
                                                   const double* __restrict__ base,
                                                   const int64_t* __restrict__ cursor,
                                                   double* __restrict__ drops) {
  const int64_t cur = *cursor;
  for (int i = threadIdx.x; i < m * b; i += 256) {
    const int sample = i % b;
    const int64_t j = cur + i / b;
    if (j < 0 || j >= nwin) continue;
    const int64_t t = target[sample];
    const double* __restrict__ row = logits + (int64_t)i * c;
    double score = __builtin_nan("");
    if (t >= 0 && t < c) {
      if (mode == MODE_LOGIT) {
        score = row[t];
      } else {
        double mx = row[0];
        for (int q = 1; q < c; ++q) mx = fmax(mx, row[q]);
        double sum = 0.0;
        for (int q = 0; q < c; ++q) sum += exp(row[q] - mx);
        score = exp(row[t] - mx) / sum;
      }
    }
    drops[j * b + sample] = base[sample] - score;
  }
}

// the windows of one axis that contain coordinate v: indices [lo, hi]
__device__ __forceinline__ void covering(int v, int s, int p, int t, int n, int* lo, int* hi) {
  // unshifted windows below lo end at or before v; the shifted last one only reaches further
  // left, and lo <= n - 1 for every v < s
  int i = v >= p ? (v - p) / t + 1 : 0;
  *lo = i;
  while (i + 1 < n && min((i + 1) * t, s - p) <= v) ++i;
  *hi = i;
}

__global__ __launch_bounds__(256) void map_kernel(Geo g, int b, int64_t total,
                                                  const double* __restrict__ drops,
                                                  float* __restrict__ map) {
  const int64_t nth = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += nth) {
    const int x = (int)(e % g.w);
    int64_t r = e / g.w;
    const int y = (int)(r % g.h);
    r /= g.h;
    const int z = (int)(r % g.d), sample = (int)(r / g.d);
    int z0, z1, y0, y1, x0, x1;
    covering(z, g.d, g.pd, g.td, g.nd, &z0, &z1);
    covering(y, g.h, g.ph, g.th, g.nh, &y0, &y1);
    covering(x, g.w, g.pw, g.tw, g.nw, &x0, &x1);
    double sum = 0.0;
    for (int iz = z0; iz <= z1; ++iz)
      for (int iy = y0; iy <= y1; ++iy)
        for (int ix = x0; ix <= x1; ++ix)
          sum += drops[((int64_t)(iz * g.nh + iy) * g.nw + ix) * b + sample];
    const int count = (z1 - z0 + 1) * (y1 - y0 + 1) * (x1 - x0 + 1);
    map[e] = (float)(sum / (double)count);
  }
}

inline bool misaligned(const void* p, uintptr_t mask) {
  return (reinterpret_cast<uintptr_t>(p) & mask) != 0;
}

}  // namespace

extern "C" {

int mmad_occlude_windows(int dtype, int b, int m, int d, int h, int w, int pd, int ph, int pw,
                         int td, int th, int tw, const void* src, void* slots,
                         const double* fill, const int64_t* cursor, int64_t nwin, void* stream) {
  if (dtype != MMAD_F64 && dtype != MMAD_F32) return MMAD_EBADDTYPE;
  if (b <= 0 || m <= 0 || (int64_t)b * m > 65535) return MMAD_EBADSHAPE;
  Geo g;
  const int rc = geo_args(d, h, w, pd, ph, pw, td, th, tw, nwin, &g);
  if (rc != MMAD_OK) return rc;
  if (!src || !slots || !fill || !cursor) return MMAD_ENULL;
  const uintptr_t emask = dtype == MMAD_F64 ? 7u : 3u;
  if (misaligned(src, emask) || misaligned(slots, emask) || misaligned(fill, 7u) ||
      misaligned(cursor, 7u))
    return MMAD_EBADSHAPE;
  const int n = dtype == MMAD_F64 ? 2 : 4;
  // every volume and every row of it starts on a 16-byte boundary, every window row is whole
  // units long; the windows' own x offsets are checked on the device
  const int vec_ok = !misaligned(src, 15u) && !misaligned(slots, 15u) && w % n == 0 && pw % n == 0;
  const int64_t items = 2 * (int64_t)pd * ph * pw;
  if (items > (int64_t(1) << 30)) return MMAD_EUNSUPPORTED;     // 32-bit item index
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(items, 256), 64), (unsigned)(b * m));
  hipStream_t st = as_stream(stream);
  if (dtype == MMAD_F64)
    hipLaunchKernelGGL((occlude_kernel<double, 2>), grid, dim3(256), 0, st, g, b, m, nwin, vec_ok,
                       static_cast<const double*>(src), static_cast<double*>(slots), fill,
                       cursor);
  else
    hipLaunchKernelGGL((occlude_kernel<float, 4>), grid, dim3(256), 0, st, g, b, m, nwin, vec_ok,
                       static_cast<const float*>(src), static_cast<float*>(slots), fill, cursor);
  return launch_status();
}

int mmad_occlusion_drop(int mode, int b, int m, int c, const double* logits,
                        const int64_t* target, const double* base, const int64_t* cursor,
                        int64_t nwin, double* drops, void* stream) {
  if (mode != MODE_LOGIT && mode != MODE_PROB) return MMAD_EBADSHAPE;
  if (b <= 0 || m <= 0 || (int64_t)b * m > 65535 || c <= 0 || c > 4096 || nwin <= 0)
    return MMAD_EBADSHAPE;
  if (!logits || !target || !base || !cursor || !drops) return MMAD_ENULL;
  if (misaligned(logits, 7u) || misaligned(target, 7u) || misaligned(base, 7u) ||
      misaligned(cursor, 7u) || misaligned(drops, 7u))
    return MMAD_EBADSHAPE;
  hipLaunchKernelGGL(drop_kernel, dim3(1), dim3(256), 0, as_stream(stream), mode, b, m, c, nwin,
                     logits, target, base, cursor, drops);
  return launch_status();
}

int mmad_occlusion_map(int b, int d, int h, int w, int pd, int ph, int pw, int td, int th,
                       int tw, const double* drops, int64_t nwin, float* map, void* stream) {
  if (b <= 0 || b > 65535) return MMAD_EBADSHAPE;
  Geo g;
  const int rc = geo_args(d, h, w, pd, ph, pw, td, th, tw, nwin, &g);
  if (rc != MMAD_OK) return rc;
  if (!drops || !map) return MMAD_ENULL;
  if (misaligned(drops, 7u) || misaligned(map, 3u)) return MMAD_EBADSHAPE;
  const int64_t total = (int64_t)b * d * h * w;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(total, 256), MAX_BLOCKS);
  hipLaunchKernelGGL(map_kernel, dim3(grid), dim3(256), 0, as_stream(stream), g, b, total, drops,
                     map);
  return launch_status();
}

}  // extern "C"
