// The table of kernel switches (switches.h): host code only, no kernels.
#include "switches.h"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace {

enum Kind { BOOL, INT };   // BOOL: stored as value != 0; INT: stored as given
struct Row {
  Sw id;
  const char* env;    // environment variable
  const char* name;   // mmad_set_kernel_variant name, nullptr: environment only
  int def;            // value when the variable is unset
  Kind kind;
};

// one row per switch, in the order of enum Sw; INTEGRATION.md carries the same table
constexpr Row kTable[] = {
  // residue-class conv: 1 where its tiles fill the CUs, 2 at any size, <= 0 off
  {SW_LATTICE, "MMAD_LATTICE", "lattice", 1, INT},
  // its plane-pair form (d = 4): 1 where it fills the CUs, 2 at any size, <= 0 the one-plane kernel
  {SW_LATTICE_ZP, "MMAD_LATTICE_ZP", "lattice_zp", 1, INT},
  // 5d^3 residue-class conv and wgrad: 1 where the blocks fill the CUs, 2 at any size, <= 0 off
  {SW_LATTICE5, "MMAD_LATTICE5", "lattice5", 1, INT},
  // dilation-2 residue-class conv: 1 where the tiles fill the CUs, 2 at any size, <= 0 off
  {SW_LATTICE8, "MMAD_LATTICE8", "lattice8", 1, INT},
  // lattice8 on the exact 16^3 grid: 1 the x-walk form, 0 the x-pair form
  {SW_L8_XWALK, "MMAD_L8_XWALK", "lattice8_xwalk", 1, BOOL},
  // lattice / lattice8 on ragged grids: > 0 on, else exact grids only
  {SW_LATTICE_RAGGED, "MMAD_LATTICE_RAGGED", nullptr, 1, INT},
  // residue-class weight gradient: > 0 on, else the row-gather wgrad_kernel
  {SW_LATTICE_WGRAD, "MMAD_LATTICE_WGRAD", nullptr, 1, INT},
  // lattice_conv_kernel: nonzero runs waves 4-7 at priority 1
  {SW_SETPRIO, "MMAD_SETPRIO", nullptr, 0, INT},
  // lattice_zp: nonzero puts two channel tiles on each XCD where the grid allows, 0 plain XCD order
  {SW_ZP_XCD2, "MMAD_ZP_XCD2", nullptr, 1, INT},
  // patch-resident conv: 1 on layers of up to 128 channels, 2 at any width, <= 0 off
  {SW_PATCH, "MMAD_PATCH", nullptr, 1, INT},
  // its output-box depth: 0 two planes (two 4-wave blocks per CU), 1 four (one 8-wave block)
  {SW_PATCH_TZ4, "MMAD_PATCH_TZ4", nullptr, 0, BOOL},
  // z-walking patch conv: 1 where the work items fill the CUs, 2 at any size, <= 0 off
  {SW_PATCHZ, "MMAD_PATCHZ", "patchz", 1, INT},
  // stride-2 sub-patch conv and its dgrad: > 0 on, else the implicit GEMM
  {SW_S2CONV, "MMAD_S2CONV", nullptr, 1, INT},
  // 1x1x1 convs as pointwise GEMMs (fwd, dgrad, wgrad): 0 the implicit GEMM
  {SW_PW_GEMM, "MMAD_PW_GEMM", nullptr, 1, BOOL},
  // the pointwise weight gradient alone: 0 the row-gather wgrad_kernel
  {SW_PW_WGRAD, "MMAD_PW_WGRAD", nullptr, 1, BOOL},
  // 16-wide stride-2 3^3 wgrad: 1 de-duplicated X rows, 0 three gathered images per stage
  {SW_PW_WG3_DEDUP, "MMAD_PW_WG3_DEDUP", "pw_wg3_dedup", 1, BOOL},
  // patch-resident weight gradient: 0 the row-gather wgrad_kernel
  {SW_PWGRAD, "MMAD_PWGRAD", nullptr, 1, BOOL},
  // its residue-class form (layer3's dilation-2 convs): 0 off
  {SW_PWGRAD_LAT, "MMAD_PWGRAD_LAT", nullptr, 1, BOOL},
  // its 16-wide form: 0 off
  {SW_PWGRAD_W16, "MMAD_PWGRAD_W16", nullptr, 1, BOOL},
  // its 40-wide form: 0 off
  {SW_PWGRAD_W40, "MMAD_PWGRAD_W40", nullptr, 1, BOOL},
  // its residue-class form: 1 keeps one class group per block, else two where that fills the CUs
  {SW_PWGRAD_LAT_NG, "MMAD_PWGRAD_LAT_NG", nullptr, 0, INT},
  // MedicalNet stem kernels: 0 the generic implicit GEMM
  {SW_STEM, "MMAD_STEM", nullptr, 1, BOOL},
  // second stem weight-gradient kernel: 0 the first
  {SW_STEM_WG2, "MMAD_STEM_WG2", nullptr, 1, BOOL},
  // quad stem forward kernel: 0 the y-pair kernel
  {SW_STEM_QUAD, "MMAD_STEM_QUAD", nullptr, 1, BOOL},
  // per-output-row fused pool kernels: 0 the grid-stride ones
  {SW_POOL_ROWS, "MMAD_POOL_ROWS", nullptr, 1, BOOL},
  // stem pool: 2 the z-walking kernel, any other value the rows kernel
  {SW_POOL_RUN, "MMAD_POOL_RUN", "pool_run", 2, INT},
  // transposing slab reduce over tap groups where the plain grid is small: 0 never
  {SW_REDUCE_TZ, "MMAD_REDUCE_TZ", nullptr, 1, BOOL},
  // 256 x 256 wgrad tiles: 0 never, > 0 wherever they fit, < 0 the M rule
  {SW_WGRAD_BIG, "MMAD_WGRAD_BIG", nullptr, -1, INT},
  // split-K count of the row-gather wgrad: > 0 forces it, else the cost model
  {SW_WGRAD_SPLITS, "MMAD_WGRAD_SPLITS", nullptr, 0, INT},
  // the same for 1x1x1 convs only
  {SW_WGRAD_1X1_SPLITS, "MMAD_WGRAD_1X1_SPLITS", nullptr, 0, INT},
  // wgrad_kernel block placement: nonzero XCD-aware, 0 launch order
  {SW_WGRAD_XCD, "MMAD_WGRAD_XCD", nullptr, 1, INT},
  // ring depth of the 1x1x1 weight gradients: 3, any other value 2
  {SW_WGRAD_1X1_NST, "MMAD_WGRAD_1X1_NST", nullptr, 3, INT},
  // large implicit-GEMM tiles: 0 the default rule, 1-6 one configuration, < 0 128 x 128 only
  {SW_IGEMM_BIG, "MMAD_IGEMM_BIG", nullptr, 0, INT},
  // default rule: smallest K that takes 256 x 256 tiles
  {SW_IGEMM_BIG_MINK, "MMAD_IGEMM_BIG_MINK", nullptr, 1024, INT},
  // default rule: fewest 256 x 256 tiles
  {SW_IGEMM_BIG_MINBLK, "MMAD_IGEMM_BIG_MINBLK", nullptr, 200, INT},
  // ring depth of the 4-wave tiles: 2 or 3 everywhere, 0 the per-conv rule
  {SW_IGEMM_NST, "MMAD_IGEMM_NST", nullptr, 0, INT},
};
static_assert(sizeof(kTable) / sizeof(kTable[0]) == SW_COUNT, "one row per Sw");
constexpr bool in_enum_order() {
  for (int i = 0; i < SW_COUNT; ++i)
    if (kTable[i].id != i) return false;
  return true;
}
static_assert(in_enum_order(), "rows follow enum Sw");

// "resolved" is the once flag, apart from the value: any integer, negative ones included, is
// cached like any other
std::once_flag g_once[SW_COUNT];
std::atomic<int> g_value[SW_COUNT];
int g_initial[SW_COUNT];   // what the environment (or the default) gave; written under g_once

int stored(const Row& r, int v) { return r.kind == BOOL ? v != 0 : v; }

}  // namespace

int sw(Sw id) {
  std::call_once(g_once[id], [id] {
    const Row& r = kTable[id];
    const char* e = getenv(r.env);
    g_initial[id] = e ? stored(r, atoi(e)) : r.def;
    g_value[id].store(g_initial[id], std::memory_order_relaxed);
  });
  return g_value[id].load(std::memory_order_relaxed);
}

// A negative v only queries -- unless it is the value the environment gave (a process started
// with its lattice switch at -1), so that "prev = set(name, v); ...; set(name, prev)" puts
// that value back too.
int sw_set(const char* name, int v) {
  if (name == nullptr) return -1;
  for (const Row& r : kTable) {
    if (r.name == nullptr || std::strcmp(name, r.name) != 0) continue;
    const int prev = sw(r.id);
    if (v >= 0 || v == g_initial[r.id])
      g_value[r.id].store(stored(r, v), std::memory_order_relaxed);
    return prev;
  }
  return -1;
}
