// Input-pipeline augmentation on device, gfx950 (float64, as the loader's volumes): random
// flip / rotation / isotropic scale / translation as ONE trilinear resample per volume, plus a
// per-sample gain and bias.  No reference counterpart: the reference augments only through
// CPU transforms (transform_mri / transform_pet, pkg/utils/dataloader.py), one 128^3 float64
// resample per sample on a loader worker.
//
//   augment_draw_kernel   one thread per sample: every random parameter from a counter hash
//                         of the device-resident seed (mix64, one stream per quantity), the
//                         only place sine and cosine are evaluated;
//   resample_kernel       out = gain * trilinear(x; theta) + bias with the coordinate and
//                         padding rules of F.affine_grid + F.grid_sample(align_corners=False);
//   elastic_draw_kernel   one thread per control-point value of the elastic lattices, from the
//                         same seed and hash;
//   deform_kernel         resample_kernel with a smooth displacement added to the sampling
//                         position: g = theta (p, 1) + 2 u(p) / size, u the trilinear
//                         interpolation of a per-sample control lattice (voxels).  The d and h
//                         parts of that interpolation are the same along an output row, so a
//                         block first reduces the lattice to one 1-D table per row it covers
//                         (LDS); a voxel then reads one table cell and spends two fused steps
//                         per component.  sample_trilinear is shared by both kernels.
//
// The resample is a memory-bound gather: 8 B written per voxel, 8 B of compulsory reads, and
// eight neighbour reads that adjacent output voxels share (served by L2; nothing is staged in
// LDS).  Lanes run along W, so every store is a coalesced row of 8-byte values; the sample
// comes from blockIdx.y, so the 12 coefficients are wave-uniform scalar loads.
#include <algorithm>

#include "common.h"

// gain * v + bias rounds the product and the sum separately (torch's `gain * x + bias`),
// and the interpolation keeps grid_sample's operation order
#pragma clang fp contract(off)

namespace {

// stream constants: one independent uniform sequence per drawn quantity
enum { S_FLIP = 0, S_ROT = 3, S_SCALE = 6, S_TRANS = 7, S_GAIN = 10,      // gain/bias: 10 + 2m, 11 + 2m
       S_ELASTIC = S_GAIN + 2 * MMAD_AUG_MAX_MOD };                      // + component (x, y, z)

// counter: the sample, or (sample << 32 | control point) for the elastic lattice
__device__ __forceinline__ double uniform01(uint64_t seed, int stream, uint64_t counter) {
  const uint64_t key = mix64(seed * 0xD1342543DE82EF95ull + (uint64_t)(stream + 1));
  return (double)(mix64(key + counter) >> 11) * 0x1p-53;                   // [0, 1)
}
__device__ __forceinline__ double in_range(double u, double lo, double hi) {
  return fmin(fmax(lo + u * (hi - lo), lo), hi);
}

__global__ void augment_draw_kernel(int nb, int D, int H, int W, mmad_augment_cfg cfg,
                                    const uint64_t* __restrict__ seed_dev,
                                    double* __restrict__ theta, double* __restrict__ intensity) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= nb) return;
  const uint64_t seed = *seed_dev;
  // cfg's per-axis fields are in tensor order (d, h, w); the matrix is over (x, y, z)
  double f[3], ang[3], t[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {            // a: 0 = x (w), 1 = y (h), 2 = z (d)
    const int c = 2 - a;
    f[a] = uniform01(seed, S_FLIP + c, n) < cfg.flip_p[c] ? -1.0 : 1.0;
    ang[a] = in_range(uniform01(seed, S_ROT + c, n), -cfg.rot_max[c], cfg.rot_max[c]);
    t[a] = in_range(uniform01(seed, S_TRANS + c, n), -cfg.trans_max[c], cfg.trans_max[c]);
  }
  const double s = in_range(uniform01(seed, S_SCALE, n), cfg.scale_lo, cfg.scale_hi);
  double sx, cx, sy, cy, sz, cz;
  sincos(ang[0], &sx, &cx);
  sincos(ang[1], &sy, &cy);
  sincos(ang[2], &sz, &cz);
  // R = Rz Ry Rx
  const double R[3][3] = {{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx},
                          {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx},
                          {-sy, cy * sx, cy * cx}};
  const double size[3] = {(double)W, (double)H, (double)D};
  double* th = theta + (int64_t)n * 12;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double a = s * R[i][j] * f[j];
      th[i * 4 + j] = i == j ? a : a * size[j] / size[i];
    }
    th[i * 4 + 3] = 2.0 * t[i] / size[i];
  }
  for (int m = 0; m < cfg.nmod; ++m) {
    double* gb = intensity + ((int64_t)n * cfg.nmod + m) * 2;
    gb[0] = in_range(uniform01(seed, S_GAIN + 2 * m, n), cfg.gain_lo[m], cfg.gain_hi[m]);
    gb[1] = in_range(uniform01(seed, S_GAIN + 2 * m + 1, n), cfg.bias_lo[m], cfg.bias_hi[m]);
  }
}

// The kernel is bound by VALU issue, not by memory (PERF_LOG.md), so everything that is the
// same for every voxel is made on the host.
struct Extent {
  int D, H, W;
  uint32_t magic_h, magic_w;       // floor(2^32 / size): division by a multiply + one fix-up
  double fd, fh, fw;               // the sizes as doubles
  double inv_d, inv_h, inv_w;      // 1 / size: no fp64 division per voxel
};

uint32_t magic_of(int d) {
  return (uint32_t)std::min<uint64_t>((uint64_t(1) << 32) / (uint64_t)d, 0xffffffffull);
}

// q = i / d, rem = i % d for i < 2^31: umulhi(i, floor(2^32 / d)) is q or q - 1
__device__ __forceinline__ uint32_t div_magic(uint32_t i, uint32_t d, uint32_t magic,
                                              uint32_t& rem) {
  uint32_t q = __umulhi(i, magic);
  uint32_t r = i - q * d;
  if (r >= d) { ++q; r -= d; }
  rem = r;
  return q;
}

// The sampling half of both resampling kernels: from the normalised sampling position g to
// the interpolated value, grid_sample's arithmetic in grid_sample's order.
template <int PAD>
__device__ __forceinline__ double sample_trilinear(const Extent& e, const double* __restrict__ src,
                                                   double gx, double gy, double gz) {
  const int D = e.D, H = e.H, W = e.W;
  // grid_sample, align_corners=False: ((g + 1) * size - 1) / 2
  double ix = ((gx + 1.0) * e.fw - 1.0) * 0.5;
  double iy = ((gy + 1.0) * e.fh - 1.0) * 0.5;
  double iz = ((gz + 1.0) * e.fd - 1.0) * 0.5;
  // border: grid_sample's clip to [0, size - 1].  zeros: far outside, every neighbour is
  // out of range whatever the exact value: pull the coordinate next to the volume so the
  // integer conversion below is defined
  const double lo = PAD == MMAD_PAD_BORDER ? 0.0 : -1.5;
  const double up = PAD == MMAD_PAD_BORDER ? -1.0 : 0.5;
  ix = fmin(fmax(ix, lo), e.fw + up);
  iy = fmin(fmax(iy, lo), e.fh + up);
  iz = fmin(fmax(iz, lo), e.fd + up);
  const double fx = floor(ix), fy = floor(iy), fz = floor(iz);
  const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
  const double wx[2] = {(fx + 1.0) - ix, ix - fx};
  const double wy[2] = {(fy + 1.0) - iy, iy - fy};
  const double wz[2] = {(fz + 1.0) - iz, iz - fz};
  // the eight loads go out together from clamped (always valid) addresses; a neighbour
  // outside the volume contributes zero (select, not a multiply: data may hold inf)
  // One multiply chain for the first neighbour's offset inside the sample (< vox < 2^31;
  // the sample's base is the 64-bit part); the others are one clamped step away per axis.
  const bool okx[2] = {(unsigned)x0 < (unsigned)W, (unsigned)(x0 + 1) < (unsigned)W};
  const bool oky[2] = {(unsigned)y0 < (unsigned)H, (unsigned)(y0 + 1) < (unsigned)H};
  const bool okz[2] = {(unsigned)z0 < (unsigned)D, (unsigned)(z0 + 1) < (unsigned)D};
  const int xc = min(max(x0, 0), W - 1), yc = min(max(y0, 0), H - 1),
            zc = min(max(z0, 0), D - 1);
  const uint32_t o000 = ((uint32_t)zc * H + yc) * W + xc;
  const uint32_t step[3] = {(x0 >= 0 && x0 + 1 < W) ? 1u : 0u,
                            (y0 >= 0 && y0 + 1 < H) ? (uint32_t)W : 0u,
                            (z0 >= 0 && z0 + 1 < D) ? (uint32_t)H * W : 0u};
  double v = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {            // grid_sample's order: x fastest, then y, then z
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    const bool ok = okx[dx] && oky[dy] && okz[dz];
    const uint32_t off = o000 + (dx ? step[0] : 0u) + (dy ? step[1] : 0u) + (dz ? step[2] : 0u);
    const double sv = src[off];
    const double wgt = wx[dx] * wy[dy] * wz[dz];
    v += ok ? sv * wgt : 0.0;
  }
  return v;
}

// one output voxel per thread; flat voxel index along W first
template <int PAD>
__global__ __launch_bounds__(256) void resample_kernel(Extent e, uint32_t vox,
                                                       const double* __restrict__ x,
                                                       const double* __restrict__ theta,
                                                       const double* __restrict__ gain_bias,
                                                       int64_t gb_stride,
                                                       double* __restrict__ out) {
  const int n = blockIdx.y;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= vox) return;
  const int D = e.D, H = e.H, W = e.W;
  uint32_t xo_, yo_;
  const uint32_t row = div_magic(i, (uint32_t)W, e.magic_w, xo_);
  const int zo = (int)div_magic(row, (uint32_t)H, e.magic_h, yo_);
  const int xo = (int)xo_, yo = (int)yo_;
  const double* __restrict__ th = theta + (int64_t)n * 12;
  double t[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) t[k] = th[k];
  const double* __restrict__ src = x + (int64_t)n * vox;
  // theta == diag(+-1) exactly, zero elsewhere (+-0): tested on the bit patterns, which keeps
  // the whole test in scalar integer instructions (the coefficients are wave-uniform)
  auto mag = [](double c) { return (uint64_t)__double_as_longlong(c) & 0x7fffffffffffffffull; };
  constexpr uint64_t ONE = 0x3ff0000000000000ull;
  const bool mirror = mag(t[0]) == ONE && mag(t[5]) == ONE && mag(t[10]) == ONE &&
                      (mag(t[1]) | mag(t[2]) | mag(t[3]) | mag(t[4]) | mag(t[6]) | mag(t[7]) |
                       mag(t[8]) | mag(t[9]) | mag(t[11])) == 0;
  double v;
  if (mirror) {                              // per sample, hence uniform over the block
    auto neg = [](double c) { return __double_as_longlong(c) < 0; };
    const int xi = neg(t[0]) ? W - 1 - xo : xo;
    const int yi = neg(t[5]) ? H - 1 - yo : yo;
    const int zi = neg(t[10]) ? D - 1 - zo : zo;
    v = src[((uint32_t)zi * H + yi) * W + xi];           // < vox < 2^31 inside the sample
  } else {
    // affine_grid: voxel centres at (2 i + 1) / size - 1, grid = theta (x, y, z, 1)
    const double xn = (double)(2 * xo + 1) * e.inv_w - 1.0;
    const double yn = (double)(2 * yo + 1) * e.inv_h - 1.0;
    const double zn = (double)(2 * zo + 1) * e.inv_d - 1.0;
    const double gx = t[0] * xn + t[1] * yn + t[2] * zn + t[3];
    const double gy = t[4] * xn + t[5] * yn + t[6] * zn + t[7];
    const double gz = t[8] * xn + t[9] * yn + t[10] * zn + t[11];
    v = sample_trilinear<PAD>(e, src, gx, gy, gz);
  }
  if (gain_bias != nullptr) {
    const double* gb = gain_bias + (int64_t)n * gb_stride;
    v = gb[0] * v + gb[1];
  }
  out[(int64_t)n * vox + i] = v;
}

// One thread per lattice value: lattice [b][3][gd][gh][gw], component c over (x, y, z), each
// value uniform in +-max of its own axis.  Keyed by (sample, component, point), so a sample's
// lattice does not depend on the batch size.
__global__ void elastic_draw_kernel(int nb, int points, double max_x, double max_y, double max_z,
                                    const uint64_t* __restrict__ seed_dev,
                                    double* __restrict__ lattice) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y, n = blockIdx.z;
  if (p >= points) return;
  const double m = c == 0 ? max_x : c == 1 ? max_y : max_z;
  const double u = uniform01(*seed_dev, S_ELASTIC + c, ((uint64_t)n << 32) | (uint64_t)p);
  lattice[((int64_t)n * 3 + c) * points + p] = in_range(u, -m, m);
}

// The lattice of the deforming resample (align_corners=True over [-1, 1]), host-made factors
struct Lattice {
  int gd, gh, gw;
  double sd, sh, sw;                        // (G - 1) / (2 size): voxel index to lattice coordinate
  double two_inv_d, two_inv_h, two_inv_w;   // 2 / size: voxels to normalised units
};

constexpr int DEFORM_ROWS = 16;                        // whole rows a block covers at most ...
constexpr int DEFORM_TABLE_ROWS = DEFORM_ROWS + 1;     // ... and the rows a 256-voxel span can touch
constexpr int LATTICE_MAX = 12;
constexpr int TABLE_ROW = (LATTICE_MAX - 1) * 6;       // doubles per row of the LDS table

// Cell and fraction of lattice coordinate (p + 1) (g - 1) / 2 on an axis of g points, for the
// centre p = (2 i + 1) / size - 1 of voxel i: (2 i + 1) * scale with scale = (g - 1) / (2 size),
// strictly inside (0, g - 1), so only the cell index is clamped (to keep every read in range).
__device__ __forceinline__ int lattice_cell(int i, double scale, int g, double& frac) {
  const double l = (double)(2 * i + 1) * scale;
  const int c = min(max((int)l, 0), g - 2);
  frac = l - (double)c;
  return c;
}

// One output voxel per thread, flat voxel index along W first as resample_kernel; a block
// covers `span` = min(256, DEFORM_ROWS * W) consecutive voxels, hence at most
// DEFORM_TABLE_ROWS output rows.  Per row and lattice cell along w, LDS holds for each
// component (a, b - a): the lattice interpolated along d and h at the cell's two ends.
template <int PAD>
__global__ __launch_bounds__(256) void deform_kernel(Extent e, Lattice g, uint32_t vox,
                                                     uint32_t span,
                                                     const double* __restrict__ x,
                                                     const double* __restrict__ theta,
                                                     const double* __restrict__ lattice,
                                                     const double* __restrict__ gain_bias,
                                                     int64_t gb_stride,
                                                     double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double table[DEFORM_TABLE_ROWS * TABLE_ROW];
  const int n = blockIdx.y;
  const int H = e.H, W = e.W;
  const uint32_t first = blockIdx.x * span;                  // < vox by the grid's size
  const uint32_t last = min(first + span, vox) - 1u;
  uint32_t rem;
  const uint32_t row0 = div_magic(first, (uint32_t)W, e.magic_w, rem);
  const int nrows = (int)(div_magic(last, (uint32_t)W, e.magic_w, rem) - row0) + 1;
  const int cells = g.gw - 1;
  const int points = g.gd * g.gh * g.gw;
  const double* __restrict__ lat = lattice + (int64_t)n * 3 * points;
  // 64 lanes a row: lane = cell * 4 + component (no division by a run-time extent); wave w
  // takes rows w, w + 4, ... (the row is wave-uniform: its index arithmetic is scalar)
  const int c = threadIdx.x & 3, cell = (threadIdx.x >> 2) & 15;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (c < 3 && cell < cells) {
    for (int r = wave; r < nrows; r += 4) {
      uint32_t yo;
      const uint32_t zo = div_magic(row0 + (uint32_t)r, (uint32_t)H, e.magic_h, yo);
      double fy, fz;
      const int cy = lattice_cell((int)yo, g.sh, g.gh, fy);
      const int cz = lattice_cell((int)zo, g.sd, g.gd, fz);
      const double* q = lat + __builtin_amdgcn_readfirstlane((cz * g.gh + cy) * g.gw) +
                        (__mul24(c, points) + cell);
      const int sy = g.gw, sz = g.gh * g.gw;
      double end[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const double v0 = fma(fy, q[j + sy] - q[j], q[j]);
        const double v1 = fma(fy, q[j + sz + sy] - q[j + sz], q[j + sz]);
        end[j] = fma(fz, v1 - v0, v0);
      }
      double* t = table + r * TABLE_ROW + cell * 6 + c * 2;
      t[0] = end[0];
      t[1] = end[1] - end[0];
    }
  }
  __syncthreads();
  const uint32_t i = first + threadIdx.x;
  if (threadIdx.x >= span || i >= vox) return;
  uint32_t xo_, yo_;
  const uint32_t row = div_magic(i, (uint32_t)W, e.magic_w, xo_);
  const int zo = (int)div_magic(row, (uint32_t)H, e.magic_h, yo_);
  const int xo = (int)xo_, yo = (int)yo_;
  const double* __restrict__ th = theta + (int64_t)n * 12;
  double t[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) t[k] = th[k];
  const double* __restrict__ src = x + (int64_t)n * vox;
  const double xn = (double)(2 * xo + 1) * e.inv_w - 1.0;
  const double yn = (double)(2 * yo + 1) * e.inv_h - 1.0;
  const double zn = (double)(2 * zo + 1) * e.inv_d - 1.0;
  double gx = t[0] * xn + t[1] * yn + t[2] * zn + t[3];
  double gy = t[4] * xn + t[5] * yn + t[6] * zn + t[7];
  double gz = t[8] * xn + t[9] * yn + t[10] * zn + t[11];
  double fx;
  const int cx = lattice_cell(xo, g.sw, g.gw, fx);
  const double* u = table + __mul24((int)(row - row0), TABLE_ROW) + __mul24(cx, 6);
  // a zero lattice leaves g as the affine kernel has it (fma(0, c, g) == g)
  gx = fma(fma(fx, u[1], u[0]), g.two_inv_w, gx);
  gy = fma(fma(fx, u[3], u[2]), g.two_inv_h, gy);
  gz = fma(fma(fx, u[5], u[4]), g.two_inv_d, gz);
  double v = sample_trilinear<PAD>(e, src, gx, gy, gz);
  if (gain_bias != nullptr) {
    const double* gb = gain_bias + (int64_t)n * gb_stride;
    v = gb[0] * v + gb[1];
  }
  out[(int64_t)n * vox + i] = v;
}

bool range_ok(double lo, double hi) { return lo <= hi; }   // false for NaN
bool lattice_ok(int gd, int gh, int gw) {
  return gd >= 2 && gd <= LATTICE_MAX && gh >= 2 && gh <= LATTICE_MAX && gw >= 2 &&
         gw <= LATTICE_MAX;
}

}  // namespace

extern "C" {

int mmad_augment_draw(int b, int d, int h, int w, const mmad_augment_cfg* cfg,
                      const uint64_t* seed, double* theta, double* intensity, void* stream) {
  if (b <= 0 || d <= 0 || h <= 0 || w <= 0) return MMAD_EBADSHAPE;
  if (!cfg || !seed || !theta || !intensity) return MMAD_ENULL;
  if (cfg->nmod < 1 || cfg->nmod > MMAD_AUG_MAX_MOD) return MMAD_EBADSHAPE;
  for (int a = 0; a < 3; ++a)
    if (!(cfg->flip_p[a] >= 0.0 && cfg->flip_p[a] <= 1.0) || !(cfg->rot_max[a] >= 0.0) ||
        !(cfg->trans_max[a] >= 0.0))
      return MMAD_EBADSHAPE;
  if (!range_ok(cfg->scale_lo, cfg->scale_hi) || !(cfg->scale_lo > 0.0)) return MMAD_EBADSHAPE;
  for (int m = 0; m < cfg->nmod; ++m)
    if (!range_ok(cfg->gain_lo[m], cfg->gain_hi[m]) || !range_ok(cfg->bias_lo[m], cfg->bias_hi[m]))
      return MMAD_EBADSHAPE;
  hipLaunchKernelGGL(augment_draw_kernel, dim3((unsigned)cdiv(b, 64)), dim3(64), 0,
                     as_stream(stream), b, d, h, w, *cfg, seed, theta, intensity);
  return launch_status();
}

int mmad_affine_resample3d(int b, int d, int h, int w, const double* x, const double* theta,
                           const double* gain_bias, int64_t gb_stride, int padding,
                           double* out, void* stream) {
  if (b <= 0 || b > 65535 || d <= 0 || h <= 0 || w <= 0 || gb_stride < 0) return MMAD_EBADSHAPE;
  const int64_t vox = (int64_t)d * h * w;
  if (vox >= (int64_t(1) << 31)) return MMAD_EUNSUPPORTED;
  if (padding != MMAD_PAD_ZEROS && padding != MMAD_PAD_BORDER) return MMAD_EUNSUPPORTED;
  if (!x || !theta || !out) return MMAD_ENULL;
  if (x == out) return MMAD_EUNSUPPORTED;          // a gather cannot run in place
  const Extent e{d, h, w, magic_of(h), magic_of(w), (double)d, (double)h, (double)w,
                 1.0 / d, 1.0 / h, 1.0 / w};
  const dim3 grid((unsigned)cdiv(vox, 256), (unsigned)b);
  if (padding == MMAD_PAD_BORDER)
    hipLaunchKernelGGL(resample_kernel<MMAD_PAD_BORDER>, grid, dim3(256), 0, as_stream(stream), e,
                       (uint32_t)vox, x, theta, gain_bias, gb_stride, out);
  else
    hipLaunchKernelGGL(resample_kernel<MMAD_PAD_ZEROS>, grid, dim3(256), 0, as_stream(stream), e,
                       (uint32_t)vox, x, theta, gain_bias, gb_stride, out);
  return launch_status();
}

int mmad_elastic_draw(int b, int gd, int gh, int gw, double max_d, double max_h, double max_w,
                      const uint64_t* seed, double* lattice, void* stream) {
  if (b <= 0 || b > 65535 || !lattice_ok(gd, gh, gw)) return MMAD_EBADSHAPE;
  if (!(max_d >= 0.0) || !(max_h >= 0.0) || !(max_w >= 0.0)) return MMAD_EBADSHAPE;   // NaN too
  if (!seed || !lattice) return MMAD_ENULL;
  const int points = gd * gh * gw;
  hipLaunchKernelGGL(elastic_draw_kernel, dim3((unsigned)cdiv(points, 64), 3u, (unsigned)b),
                     dim3(64), 0, as_stream(stream), b, points, max_w, max_h, max_d, seed, lattice);
  return launch_status();
}

int mmad_deform_resample3d(int b, int d, int h, int w, const double* x, const double* theta,
                           int gd, int gh, int gw, const double* lattice,
                           const double* gain_bias, int64_t gb_stride, int padding,
                           double* out, void* stream) {
  if (b <= 0 || b > 65535 || d <= 0 || h <= 0 || w <= 0 || gb_stride < 0) return MMAD_EBADSHAPE;
  if (!lattice_ok(gd, gh, gw)) return MMAD_EBADSHAPE;
  const int64_t vox = (int64_t)d * h * w;
  if (vox >= (int64_t(1) << 31)) return MMAD_EUNSUPPORTED;
  if (padding != MMAD_PAD_ZEROS && padding != MMAD_PAD_BORDER) return MMAD_EUNSUPPORTED;
  if (!x || !theta || !lattice || !out) return MMAD_ENULL;
  if (x == out) return MMAD_EUNSUPPORTED;          // a gather cannot run in place
  const Extent e{d, h, w, magic_of(h), magic_of(w), (double)d, (double)h, (double)w,
                 1.0 / d, 1.0 / h, 1.0 / w};
  const Lattice g{gd, gh, gw, 0.5 * (gd - 1) / d, 0.5 * (gh - 1) / h, 0.5 * (gw - 1) / w,
                  2.0 / d, 2.0 / h, 2.0 / w};
  const uint32_t span = (uint32_t)std::min<int64_t>(256, (int64_t)DEFORM_ROWS * w);
  const dim3 grid((unsigned)cdiv(vox, span), (unsigned)b);
  if (padding == MMAD_PAD_BORDER)
    hipLaunchKernelGGL(deform_kernel<MMAD_PAD_BORDER>, grid, dim3(256), 0, as_stream(stream), e, g,
                       (uint32_t)vox, span, x, theta, lattice, gain_bias, gb_stride, out);
  else
    hipLaunchKernelGGL(deform_kernel<MMAD_PAD_ZEROS>, grid, dim3(256), 0, as_stream(stream), e, g,
                       (uint32_t)vox, span, x, theta, lattice, gain_bias, gb_stride, out);
  return launch_status();
}

}  // extern "C"
