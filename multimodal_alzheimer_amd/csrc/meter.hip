// Epoch meter, gfx950 (metrics.EpochMeter): the per-epoch loss mean, confusion matrix, macro /
// per-class F1, MCC and accuracy of Base_Model's *_epoch_end hooks
// (pkg/models/base_model.py:91-149) and the rows test_epoch_end concatenates for
// bootstrap_metric (:151-174), accumulated on the device.  The reference updates torchmetrics
// objects from Python on every step and keeps a Python list of every step's outputs; a
// captured step can do neither, so one one-block launch per step folds the step's logits,
// labels and loss into a small state buffer (layout: include/mmad.h), and one more per epoch
// evaluates it.  Nothing is read by the host; both launches are capturable.
//
// One block on purpose: a batch is at most a few hundred rows of <= 16 logits, and a single
// block owns the state, so the matrix is counted in LDS (integer adds: any order gives the same
// counts) and added to the global one without cross-block atomics, and the loss partials are
// summed in thread order exactly as loss_kernel (head.hip) sums them.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int METER_MAXC = 16;              // BOOT_MAXC of head.hip
// eight-byte slots of the state (metrics.py exports the same names)
enum { M_SEEN = 0, M_COUNTED, M_BATCHES, M_LIMIT, M_BAD_LABELS, M_OVERFLOW, M_LOSS_SUM,
       M_LOSS_LAST, M_CM };

template <typename TI>
__global__ __launch_bounds__(NT) void meter_update_kernel(
    int B, int C, const TI* __restrict__ xin, const int64_t* __restrict__ y,
    const double* __restrict__ loss_in, const double* __restrict__ w, double gamma, int mode,
    int64_t* state, double* __restrict__ rows_logits,
    int64_t* __restrict__ rows_labels, int64_t cap) {
  __shared__ int cm[METER_MAXC * METER_MAXC];
  __shared__ int bad;
  __shared__ double red[2][NT];
  struct Wide {
    const TI* p;
    __device__ double operator[](int64_t i) const { return (double)p[i]; }
  } x{xin};
  // every thread reads the counters before thread 0 rewrites them behind the barriers below
  const int64_t seen = state[M_SEEN], limit = state[M_LIMIT], counted0 = state[M_COUNTED];
  int64_t left = limit < 0 ? (int64_t)B : limit - seen;
  left = left < 0 ? 0 : left;
  const int valid = left < B ? (int)left : B;
  for (int i = threadIdx.x; i < C * C; i += NT) cm[i] = 0;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < valid; b += NT) {
    int p = 0;
    double best = x[(int64_t)b * C];
    for (int c = 1; c < C; ++c) {
      const double v = x[(int64_t)b * C + c];
      if (v > best || (v != v && best == best)) { best = v; p = c; }
    }
    const int64_t t = y[b];
    if (t >= 0 && t < C) atomicAdd(&cm[(int)t * C + p], 1);
    else atomicAdd(&bad, 1);
    const int64_t r = counted0 + b;
    if (rows_logits != nullptr && r < cap) {
      for (int c = 0; c < C; ++c) rows_logits[r * C + c] = x[(int64_t)b * C + c];
      rows_labels[r] = t;
    }
  }
  // the batch loss over rows [0, valid): loss_kernel's arithmetic and summation order
  // (head.hip; at most NT threads there too, sample b on thread b % NT)
  const bool given = loss_in != nullptr && valid == B;
  double num = 0.0, den = 0.0;
  if (!given && valid > 0 && mode >= 0) {
    const int igamma = (int)gamma;
    const bool int_gamma = (double)igamma == gamma && igamma >= 0 && igamma <= 16;
    for (int b = threadIdx.x; b < valid; b += NT) {
      const int64_t t = y[b];
      if (t < 0 || t >= C) continue;
      double mx = -__builtin_inf();
      for (int c = 0; c < C; ++c) mx = fmax(mx, x[(int64_t)b * C + c]);
      double se = 0.0;
      for (int c = 0; c < C; ++c) se += exp(x[(int64_t)b * C + c] - mx);
      const double lse = mx + log(se);
      const double logpt = x[(int64_t)b * C + t] - lse;
      if (mode == 0) {
        const double wt = w ? w[t] : 1.0;
        num += wt * -logpt;
        den += wt;
      } else {
        const double pt = exp(logpt);
        double f;
        if (int_gamma) { f = 1.0; for (int k = 0; k < igamma; ++k) f *= (1.0 - pt); }
        else f = pow(1.0 - pt, gamma);
        num += -f * logpt;
        den += 1.0;
      }
    }
  }
  red[0][threadIdx.x] = num;
  red[1][threadIdx.x] = den;
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += NT)
    if (cm[i] != 0) state[M_CM + i] += cm[i];
  if (threadIdx.x != 0) return;
  state[M_SEEN] = seen + B;
  if (valid == 0) return;
  state[M_COUNTED] = counted0 + valid;
  state[M_BATCHES] += 1;
  state[M_BAD_LABELS] += bad;
  if (rows_logits != nullptr) {
    const int64_t room = cap > counted0 ? cap - counted0 : 0;
    if (valid > room) state[M_OVERFLOW] += valid - room;
  }
  double loss;
  if (given) {
    loss = *loss_in;
  } else if (mode >= 0) {
    double a = 0.0, d = 0.0;
    const int nk = min(NT, valid);
    for (int k = 0; k < nk; ++k) { a += red[0][k]; d += red[1][k]; }
    loss = a / d;
  } else {
    loss = __builtin_nan("");
  }
  // (the two doubles live in int64 slots: moved as bits)
  state[M_LOSS_SUM] = __double_as_longlong(__longlong_as_double(state[M_LOSS_SUM]) + loss);
  state[M_LOSS_LAST] = __double_as_longlong(loss);
}

// out[0 .. 3 + C]: mean batch loss, macro F1, MCC, accuracy, per-class F1 -- bootstrap_kernel's
// definitions (head.hip) on the int64 matrix, kept in f64
__global__ void meter_compute_kernel(int C, const int64_t* __restrict__ state,
                                     double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const int64_t* cm = state + M_CM;
  const double loss_sum = __longlong_as_double(state[M_LOSS_SUM]);
  out[0] = loss_sum / (double)state[M_BATCHES];
  double f1sum = 0.0;
  int used = 0;
  double s = 0.0, tr = 0.0, tp_sum = 0.0, pp = 0.0, tt = 0.0;
  for (int c = 0; c < C; ++c) {
    double tk = 0.0, pk = 0.0;
    for (int j = 0; j < C; ++j) { tk += (double)cm[c * C + j]; pk += (double)cm[j * C + c]; }
    const double tp = (double)cm[c * C + c], fp = pk - tp, fn = tk - tp;
    double f1 = 0.0;
    if (tp + fp + fn > 0) { f1 = 2.0 * tp / (2.0 * tp + fp + fn); f1sum += f1; ++used; }
    out[4 + c] = f1;
    s += tk; tr += tp; tp_sum += tk * pk; pp += pk * pk; tt += tk * tk;
  }
  out[1] = used ? f1sum / used : 0.0;
  const double cov_tp = tr * s - tp_sum, cov_pp = s * s - pp, cov_tt = s * s - tt;
  out[2] = cov_pp * cov_tt == 0.0 ? 0.0 : cov_tp / sqrt(cov_tt * cov_pp);
  out[3] = s > 0.0 ? tr / s : 0.0;
}

bool misaligned(const void* p, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0;
}

}  // namespace

extern "C" {

int mmad_meter_update(int b, int c, int logits_dtype, const void* logits, const int64_t* labels,
                      const double* loss_in, const double* w, double gamma, int mode,
                      void* state, double* rows_logits, int64_t* rows_labels, int64_t cap,
                      void* stream) {
  if (b <= 0 || c <= 0 || c > METER_MAXC || mode < -1 || mode > 1) return MMAD_EBADSHAPE;
  if (logits_dtype != MMAD_F32 && logits_dtype != MMAD_F64) return MMAD_EBADDTYPE;
  if (!logits || !labels || !state) return MMAD_ENULL;
  if ((rows_logits == nullptr) != (rows_labels == nullptr)) return MMAD_ENULL;
  if (rows_logits != nullptr && cap <= 0) return MMAD_EBADSHAPE;
  if (misaligned(logits, logits_dtype == MMAD_F64 ? 8 : 4) || misaligned(labels, 8) ||
      misaligned(loss_in, 8) || misaligned(w, 8) || misaligned(state, 8) ||
      misaligned(rows_logits, 8) || misaligned(rows_labels, 8))
    return MMAD_EBADSHAPE;
  hipStream_t st = as_stream(stream);
  if (logits_dtype == MMAD_F64)
    hipLaunchKernelGGL(meter_update_kernel<double>, dim3(1), dim3(NT), 0, st, b, c,
                       (const double*)logits, labels, loss_in, w, gamma, mode, (int64_t*)state,
                       rows_logits, rows_labels, cap);
  else
    hipLaunchKernelGGL(meter_update_kernel<float>, dim3(1), dim3(NT), 0, st, b, c,
                       (const float*)logits, labels, loss_in, w, gamma, mode, (int64_t*)state,
                       rows_logits, rows_labels, cap);
  return launch_status();
}

int mmad_meter_compute(int c, const void* state, double* out, void* stream) {
  if (c <= 0 || c > METER_MAXC) return MMAD_EBADSHAPE;
  if (!state || !out) return MMAD_ENULL;
  if (misaligned(state, 8) || misaligned(out, 8)) return MMAD_EBADSHAPE;
  hipLaunchKernelGGL(meter_compute_kernel, dim3(1), dim3(64), 0, as_stream(stream), c,
                     (const int64_t*)state, out);
  return launch_status();
}

}  // extern "C"
