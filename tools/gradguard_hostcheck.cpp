// Host-side check of the gradient guard's entry points (csrc/gradguard.hip, and
// mmad_adam_repack_guarded in csrc/adam.hip) for a sanitizer build: fills a mmad_grad_job table
// the way fused_optim.GradGuard does and walks every argument check that returns before a
// launch.  No kernel is launched and no device is needed.
//
//   hipcc -O1 -g -std=c++20 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       tools/gradguard_hostcheck.cpp multimodal_alzheimer_amd/csrc/gradguard.hip \
//       multimodal_alzheimer_amd/csrc/adam.hip -o build/gradguard_hostcheck
//   build/gradguard_hostcheck
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/mmad.h"

#define CHECK(expr, want)                                                     \
  do {                                                                        \
    const long long got_ = (long long)(expr);                                 \
    if (got_ != (long long)(want)) {                                          \
      std::fprintf(stderr, "%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #expr, got_, \
                   (long long)(want));                                        \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

int main() {
  // a job table over gradients of these sizes, in 4096-element chunks
  const int64_t sizes[] = {64 * 64 * 27, 128 * 64, 64, 2, 35, 1000, 4099, 1};
  std::vector<float> storage(4099 + 1);
  std::vector<mmad_grad_job> jobs;
  int64_t chunks = 0;
  for (int64_t n : sizes) {
    mmad_grad_job j;
    j.grad = storage.data() + (n == 4099 ? 1 : 0);     // never dereferenced by the host
    j.numel = n;
    j.chunk0 = chunks;
    chunks += (n + 4095) / 4096;
    jobs.push_back(j);
  }
  CHECK(chunks, 27 + 2 + 1 + 1 + 1 + 1 + 2 + 1);
  CHECK(mmad_grad_guard_blocks(chunks), chunks);
  CHECK(mmad_grad_guard_blocks(0), 0);
  CHECK(mmad_grad_guard_blocks(-5), 0);
  CHECK(mmad_grad_guard_blocks(1), 1);
  CHECK(mmad_grad_guard_blocks(1024), 1024);
  CHECK(mmad_grad_guard_blocks(5000), 1024);
  CHECK(mmad_grad_guard_blocks((int64_t)1 << 40), 1024);

  std::vector<double> partials(1024), state(10);
  std::vector<int> arrivals(jobs.size());
  std::vector<mmad_adam_job> ajobs(2);
  const int nj = (int)jobs.size();
  const int nb = mmad_grad_guard_blocks(chunks);
  // nothing to do
  CHECK(mmad_grad_sumsq(0, nullptr, 0, 0, nullptr, nullptr), MMAD_OK);
  CHECK(mmad_grad_sumsq(-1, jobs.data(), chunks, nb, partials.data(), nullptr), MMAD_OK);
  CHECK(mmad_grad_sumsq(nj, jobs.data(), 0, nb, partials.data(), nullptr), MMAD_OK);
  CHECK(mmad_grad_scale(0, nullptr, 0, nullptr, nullptr), MMAD_OK);
  CHECK(mmad_adam_repack_guarded(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr), MMAD_OK);
  // null pointers
  CHECK(mmad_grad_sumsq(nj, nullptr, chunks, nb, partials.data(), nullptr), MMAD_ENULL);
  CHECK(mmad_grad_sumsq(nj, jobs.data(), chunks, nb, nullptr, nullptr), MMAD_ENULL);
  CHECK(mmad_grad_guard_finalize(nb, nullptr, state.data(), nullptr), MMAD_ENULL);
  CHECK(mmad_grad_guard_finalize(nb, partials.data(), nullptr, nullptr), MMAD_ENULL);
  CHECK(mmad_grad_scale(nj, nullptr, chunks, state.data(), nullptr), MMAD_ENULL);
  CHECK(mmad_grad_scale(nj, jobs.data(), chunks, nullptr, nullptr), MMAD_ENULL);
  CHECK(mmad_adam_repack_guarded(2, ajobs.data(), nullptr, 3, arrivals.data(), nullptr, nullptr),
        MMAD_ENULL);
  CHECK(mmad_adam_repack_guarded(2, nullptr, nullptr, 3, arrivals.data(), state.data(), nullptr),
        MMAD_ENULL);
  CHECK(mmad_adam_repack_guarded(2, ajobs.data(), nullptr, 3, nullptr, state.data(), nullptr),
        MMAD_ENULL);
  // work to do and no block for it, or more blocks than partials has slots
  CHECK(mmad_grad_sumsq(nj, jobs.data(), chunks, 0, partials.data(), nullptr), MMAD_EBADSHAPE);
  CHECK(mmad_grad_sumsq(nj, jobs.data(), chunks, -3, partials.data(), nullptr), MMAD_EBADSHAPE);
  CHECK(mmad_grad_sumsq(nj, jobs.data(), 5000, 1025, partials.data(), nullptr), MMAD_EBADSHAPE);
  CHECK(mmad_grad_guard_finalize(-1, partials.data(), state.data(), nullptr), MMAD_EBADSHAPE);
  CHECK(mmad_grad_guard_finalize(1025, partials.data(), state.data(), nullptr), MMAD_EBADSHAPE);
  std::puts("gradguard host checks ok");
  return 0;
}
