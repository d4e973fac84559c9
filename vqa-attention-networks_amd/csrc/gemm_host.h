// Host-side launch rules shared by the GEMM translation units (gemm_f32*.hip, gemm_bf16*.hip).  HOST ONLY: nothing here reaches
// a kernel.  What a family decides for itself stays in its file: which shapes it takes (big_applies, whole_round_rows,
// streamk_tail, the per-wave kernel's round test), the two pick_splits cost models, deal_edge_tiles, every measured threshold.
#pragma once
#include <algorithm>
#include "common.h"

// Launch a kernel that takes its arguments as ONE by-value struct and asks for dynamic LDS: the attribute once per device and
// kernel (common.h, vqf_set_dyn_lds: the flags are a static of this instantiation, i.e. per kernel instantiation), the launch
// with the profiler's brackets, the launch status.
template <auto Kernel, typename Args>
static inline int vqf_launch_dyn_lds(int kid, dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const Args& g) {
  static VqfDynLdsFlags attr = {};
  if (int e = vqf_set_dyn_lds(reinterpret_cast<const void*>(Kernel), lds_bytes, attr)) return e;
  VQF_LAUNCH(kid, Kernel, grid, block, lds_bytes, s, g);
  return vqf_last_error();
}

// A run-time flag as a compile-time constant: f(std::true_type()) or f(std::false_type()); evaluates to what f returns.
// FIRST: the value whose branch is written, and so instantiated, first.  The kernels of a code object lie in the order of their
// instantiation; the 128x128-tile files have always held theirs false-first, the other families true-first, and stay so.
template <bool FIRST = true, typename F> static inline int vqf_dispatch_bool(int flag, F&& f) {
  return (flag != 0) == FIRST ? f(std::bool_constant<FIRST>()) : f(std::bool_constant<!FIRST>());
}
// ... and the (ta, tb) pair of a product: f(TA, TB), a generic lambda that names its kernel as kernel<TA(), TB()>
template <bool FIRST = true, typename F> static inline int vqf_dispatch_ta_tb(int ta, int tb, F&& f) {
  return vqf_dispatch_bool<FIRST>(ta, [&](auto TA) { return vqf_dispatch_bool<FIRST>(tb, [&](auto TB) { return f(TA, TB); }); });
}
static inline int vqf_gemm_kid(int ta, int tb) { return KID_GEMM_A0B0 + 2 * (ta ? 1 : 0) + (tb ? 1 : 0); }

// Workgroups of a persistent launch over `items` work items: one per CU, at most VQF_OPT_GEMM_CU_LIMIT of them (that option
// leaves part of the chip to other streams); !persist (the family's persist option is off): one workgroup per item.
// whole_xcds (the large-tile kernels): the CU count is rounded down to a multiple of 8, which keeps every workgroup's items on
// its own XCD, and a chip of fewer than 8 CUs -- or an unknown one -- gets one workgroup per item; without it (the per-sample
// kernel) the count is taken as it is.
static inline int vqf_persistent_grid(int items, bool persist, bool whole_xcds) {
  if (!persist) return items;
  int cus = whole_xcds ? vqf_cu_count() & ~7 : vqf_cu_count();
  const int lim = vqf_opt(VQF_OPT_GEMM_CU_LIMIT, 0) & ~7;
  if (lim >= 8 && lim < cus) cus = lim;
  if (whole_xcds) return (cus >= 8 && items > cus) ? cus : items;
  return items < cus ? items : cus;
}

// Split-K in whole slabs of `slab_k`: the wanted split count becomes the K range of a split (*kchunk, a multiple of slab_k) and
// the number of splits that are not empty (the return value, <= wanted).
static inline int vqf_splitk_chunks(int K, int slab_k, int wanted, int* kchunk) {
  const int slabs = (K + slab_k - 1) / slab_k;
  const int per = (slabs + wanted - 1) / wanted;
  *kchunk = per * slab_k;
  return (K + *kchunk - 1) / *kchunk;
}

// After a split-K launch of status rc: a launch that failed may not have run its last arrivers, so its `words` counters are
// cleared (gemm_f32.hip, vqf_splitk_counters); one that ran without counters is followed by the reduce launch over its slabs.
static inline int vqf_splitk_finish(int rc, int* cnt, int words, const float* slab, int splits, int M, int N, float* C, int ldc,
                                    const float* bias, int flags, hipStream_t s) {
  if (rc != VQF_OK) {
    vqf_splitk_counters_clear(cnt, words, s);
    return rc;
  }
  if (splits > 1 && !cnt) rc = vqf_splitk_reduce(slab, splits, M, N, C, ldc, bias, flags, s);
  return rc;
}

// Split count of the 128x128-tile kernels (gemm_f32.hip, gemm_bf16.hip; each file keeps its own gate in front).  Two workgroups
// per CU already keep the matrix pipe busy (the others only cover bubbles), so the wave-quantisation model uses 512 slots;
// measured: img_conv1d wgrad (640 tiles) 134 TF at 4 splits vs 124 TF at 8.
static inline int vqf_tile128_splits(long long tiles, int ktiles, int M, int N, size_t ws_bytes) {
  const int slots = 512;
  int splits = 1;
  double best = 1e30;
  for (int sp = 1; sp <= 16; ++sp) {
    if (ktiles / sp < 16) break;
    if ((size_t)sp * M * N * sizeof(float) > ws_bytes) break;
    const double blocks = (double)tiles * sp;
    const double rounds = (double)((long long)((blocks + slots - 1) / slots));
    // time ~ rounds * (per-block work ~ 1/sp) ; small penalty per split for the reduce pass
    const double cost = rounds / sp * (1.0 + 0.01 * sp);
    if (cost < best - 1e-12) { best = cost; splits = sp; }
  }
  return splits;
}

// Row tiles per group of the large-tile kernels' tile order.  An XCD (private L2) works on a contiguous run of the order: the
// ~32 tiles resident at a time when one split covers the chip, or its tiles / 8 share of EACH split for the few-tile split-K
// launches (the image projection's weight gradient: 160 tiles -> 20 per XCD and split).  A run of `share` tiles
// walked row-tile-fastest in groups of gm covers gm A panels + share / gm B panels: pick the gm in 4..8 that minimises
// that, preferring one that divides the run (5 x 4 for the weight gradient: 12.3 -> 10.0 GB beyond L2, PMC).
static inline int vqf_pick_group_m(int tiles_m, int tiles_n, int splits) {
  const int ntiles = tiles_m * tiles_n;
  const int share = (splits > 1 && ntiles / 8 < 32) ? (ntiles / 8 > 0 ? ntiles / 8 : 1) : 32;
  int best = 8, best_cost = 1 << 30;
  for (int gm = 8; gm >= 4; --gm) {
    const int cost = 4 * (gm + (share + gm - 1) / gm) + (share % gm ? 2 : 0) + (tiles_m % gm ? 1 : 0);
    if (cost < best_cost) { best_cost = cost; best = gm; }
  }
  return best;
}
// The "joint" split-K work order of the large-tile kernels (option gemm_splitk_order = 1): an XCD's 32 CUs take group_m row
// tiles x all column tiles of one split.  Returns 1 and replaces *group_m where it applies (the column tiles divide 32).
static inline int vqf_splitk_joint_order(int tiles_m, int tiles_n, int splits, int* group_m) {
  if (!(splits > 1 && tiles_n <= 32 && 32 % tiles_n == 0 && vqf_opt(VQF_OPT_GEMM_SPLITK_ORDER, 0) == 1)) return 0;
  *group_m = std::min(tiles_m, 32 / tiles_n);
  return 1;
}
