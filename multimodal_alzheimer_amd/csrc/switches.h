// Every kernel switch of libmmad_hip.so: one table (switches.hip), one reader, one run-time
// setter.  A switch is an integer read from its MMAD_* environment variable the first time
// its value is asked for, and cached for the process; the eight that have a run-time name can
// also be set through mmad_set_kernel_variant.  What a value means is decided where it is
// used: the kernels' own files and conv.hip's route resolver.
#pragma once

enum Sw {   // row order of the table in switches.hip
  SW_LATTICE, SW_LATTICE_ZP, SW_LATTICE5, SW_LATTICE8, SW_L8_XWALK, SW_LATTICE_RAGGED,
  SW_LATTICE_WGRAD, SW_SETPRIO, SW_ZP_XCD2,
  SW_PATCH, SW_PATCH_TZ4, SW_PATCHZ, SW_S2CONV,
  SW_PW_GEMM, SW_PW_WGRAD, SW_PW_WG3_DEDUP,
  SW_PWGRAD, SW_PWGRAD_LAT, SW_PWGRAD_W16, SW_PWGRAD_W40, SW_PWGRAD_LAT_NG,
  SW_STEM, SW_STEM_WG2, SW_STEM_QUAD,
  SW_POOL_ROWS, SW_POOL_RUN,
  SW_REDUCE_TZ, SW_WGRAD_BIG, SW_WGRAD_SPLITS, SW_WGRAD_1X1_SPLITS, SW_WGRAD_XCD,
  SW_WGRAD_1X1_NST,
  SW_IGEMM_BIG, SW_IGEMM_BIG_MINK, SW_IGEMM_BIG_MINBLK, SW_IGEMM_NST,
  SW_COUNT
};

// the switch's value: its environment variable (read once, on the first call for this id) or
// its default, unless set at run time since
int sw(Sw id);

// mmad_set_kernel_variant: the previous value of the switch with this run-time name, which
// becomes v when v >= 0; -1 for a null name or one no row carries (the environment-only
// switches feed workspace sizes and must not move between a query and a call)
int sw_set(const char* name, int v);
