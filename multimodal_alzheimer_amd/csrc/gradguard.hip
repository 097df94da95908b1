// Gradient guard of the captured training step, gfx950 (fused_optim.GradGuard): one pass over
// the step's gradients gives their global L2 norm, the clip coefficient of
// torch.nn.utils.clip_grad_norm_ and a non-finite flag, all on the device; the fused Adam
// (adam.hip, mmad_adam_repack_guarded) consumes the coefficient and the flag, and
// mmad_grad_scale applies the coefficient in place for hand-written loops.
//
// Every gradient is cut into flat chunks of CHUNK elements (mmad_grad_job.chunk0 = the job's
// first chunk in the launch); block b of a bounded grid takes chunks b, b + nblocks, ... in
// that order.  Every product and every sum is a double from the first one on: a product of two
// floats is exact in a double and a sum of finite squares cannot overflow one, so the sum is
// non-finite exactly when some element is Inf or NaN -- no second pass, no flag traffic.  A
// thread's elements, the shuffle / LDS tree of a block and the index-order fold of the block
// partials (a second launch: the kernel boundary orders them) are all fixed by the job table and
// nblocks, so the result is bitwise reproducible whatever order the blocks run in.  No atomics.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = 4096;               // elements per chunk
constexpr int MAX_BLOCKS = 1024;          // grid bound = slots of `partials`

// slots of the float64[10] state (fused_optim exports the same names)
enum { S_MAX_NORM = 0, S_SKIP_NONFINITE, S_SUMSQ, S_NORM, S_COEF, S_SKIP, S_STEPS, S_CLIPPED,
       S_SKIPPED, S_RESERVED, S_SLOTS };

// the job of chunk c: the last one with chunk0 <= c (a block's chunks ascend, so the search
// starts at the previous chunk's job)
__device__ __forceinline__ int job_of(const mmad_grad_job* __restrict__ jobs, int lo, int njobs,
                                      int64_t c) {
  int hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// chunk c of job jb as (pointer, head, vectors, tail): `head` scalar elements up to the first
// 16-byte boundary, `nv` 16-byte vectors, `tail` scalar elements; false when the table does not
// cover the chunk
struct Span {
  int64_t e0;
  int head, nv, tail;
};
__device__ __forceinline__ bool span_of(const mmad_grad_job& jb, int64_t c, Span& s) {
  s.e0 = (c - jb.chunk0) * CHUNK;
  if (s.e0 < 0 || s.e0 >= jb.numel) return false;
  const int64_t left = jb.numel - s.e0;
  const int n = left < CHUNK ? (int)left : CHUNK;
  const uintptr_t a = reinterpret_cast<uintptr_t>(jb.grad + s.e0);
  s.head = min(n, (int)(((16 - (a & 15)) & 15) >> 2));
  s.nv = (n - s.head) >> 2;
  s.tail = n - s.head - s.nv * 4;
  return true;
}

__global__ __launch_bounds__(NT) void grad_sumsq_kernel(const mmad_grad_job* __restrict__ jobs,
                                                        int njobs, int64_t total_chunks,
                                                        double* __restrict__ partials) {
  __shared__ double red[NT / 64];
  const int t = threadIdx.x;
  double acc = 0.0;
  int lo = 0;
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    lo = job_of(jobs, lo, njobs, c);
    const mmad_grad_job jb = jobs[lo];
    Span s;
    if (!span_of(jb, c, s)) continue;
    const float* __restrict__ g = jb.grad + s.e0;
    if (t < s.head) {
      const double x = g[t];
      acc += x * x;
    }
    const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + s.head);
    // (a full chunk is NT * 4 vectors: four independent 16-byte loads per lane in flight)
#pragma unroll 4
    for (int v = t; v < s.nv; v += NT) {
      const f32x4 q = gv[v];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double x = q[i];
        acc += x * x;
      }
    }
    if (t < s.tail) {
      const double x = g[s.head + s.nv * 4 + t];
      acc += x * x;
    }
  }
  acc = wave_sum_d(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(NT) void grad_finalize_kernel(int nblocks,
                                                           const double* __restrict__ partials,
                                                           double* __restrict__ state) {
  __shared__ double part[MAX_BLOCKS];
  for (int i = threadIdx.x; i < nblocks; i += NT) part[i] = partials[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sumsq = 0.0;
#pragma unroll 8
  for (int i = 0; i < nblocks; ++i) sumsq += part[i];          // index order
  const double norm = sqrt(sumsq);
  // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0) in the
  // gradients' float32, from the float32 norm (a NaN stays a NaN, as clamp keeps it)
  const float c = (float)state[S_MAX_NORM] / ((float)norm + 1e-6f);
  const float coef = c > 1.0f ? 1.0f : c;
  const bool nonfinite = !isfinite(sumsq);
  const bool skip = nonfinite && state[S_SKIP_NONFINITE] != 0.0;
  state[S_SUMSQ] = sumsq;
  state[S_NORM] = norm;
  state[S_COEF] = (double)coef;
  state[S_SKIP] = skip ? 1.0 : 0.0;
  state[S_STEPS] += 1.0;
  if (coef < 1.0f) state[S_CLIPPED] += 1.0;
  if (skip) state[S_SKIPPED] += 1.0;
  state[S_RESERVED] = 0.0;
}

__global__ __launch_bounds__(NT) void grad_scale_kernel(const mmad_grad_job* __restrict__ jobs,
                                                        int njobs, int64_t total_chunks,
                                                        const double* __restrict__ state) {
  if (state[S_SKIP] != 0.0) return;                 // (block-uniform)
  const float coef = (float)state[S_COEF];
  if (coef == 1.0f) return;                         // g * 1.0f is g
  const int t = threadIdx.x;
  int lo = 0;
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    lo = job_of(jobs, lo, njobs, c);
    const mmad_grad_job jb = jobs[lo];
    Span s;
    if (!span_of(jb, c, s)) continue;
    float* g = const_cast<float*>(jb.grad) + s.e0;
    if (t < s.head) g[t] = __fmul_rn(g[t], coef);
    f32x4* gv = reinterpret_cast<f32x4*>(g + s.head);
#pragma unroll 4
    for (int v = t; v < s.nv; v += NT) {
      f32x4 q = gv[v];
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = __fmul_rn(q[i], coef);
      gv[v] = q;
    }
    if (t < s.tail) {
      float* e = g + s.head + s.nv * 4 + t;
      *e = __fmul_rn(*e, coef);
    }
  }
}

}  // namespace

extern "C" {

int mmad_grad_guard_blocks(int64_t total_chunks) {
  if (total_chunks <= 0) return 0;
  return total_chunks < MAX_BLOCKS ? (int)total_chunks : MAX_BLOCKS;
}

int mmad_grad_sumsq(int njobs, const mmad_grad_job* jobs_device, int64_t total_chunks,
                    int nblocks, double* partials, void* stream) {
  if (njobs <= 0 || total_chunks <= 0) return MMAD_OK;
  if (jobs_device == nullptr || partials == nullptr) return MMAD_ENULL;
  if (nblocks <= 0 || nblocks > MAX_BLOCKS) return MMAD_EBADSHAPE;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nblocks), dim3(NT), 0, as_stream(stream),
                     jobs_device, njobs, total_chunks, partials);
  return launch_status();
}

int mmad_grad_guard_finalize(int nblocks, const double* partials, double* state, void* stream) {
  if (state == nullptr || (nblocks > 0 && partials == nullptr)) return MMAD_ENULL;
  if (nblocks < 0 || nblocks > MAX_BLOCKS) return MMAD_EBADSHAPE;
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(NT), 0, as_stream(stream), nblocks,
                     partials, state);
  return launch_status();
}

int mmad_grad_scale(int njobs, const mmad_grad_job* jobs_device, int64_t total_chunks,
                    const double* state, void* stream) {
  if (njobs <= 0 || total_chunks <= 0) return MMAD_OK;
  if (jobs_device == nullptr || state == nullptr) return MMAD_ENULL;
  hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)mmad_grad_guard_blocks(total_chunks)),
                     dim3(NT), 0, as_stream(stream), jobs_device, njobs, total_chunks, state);
  return launch_status();
}

}  // extern "C"
