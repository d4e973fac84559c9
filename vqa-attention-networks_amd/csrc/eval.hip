// Evaluation tail of the solver (solver.py:96-101, 148-153) for the soft-target models, and top-k answers.
//
//  * answer match (mhb / mhb_coAtt, KL criterion): one block per row takes the arg-max of the log-probs and of the soft target in
//    ONE pass over both rows and reads the soft score of the predicted answer; a single-block kernel adds hits and scores in a
//    fixed order (no atomics) into totals that a validation epoch keeps on the device.
//  * top-k: one block per row holds the row in LDS and makes k rounds of a block arg-max; round j takes the largest
//    (value, index) key BELOW round j-1's winner, so nothing is knocked out and equal values come out in index order.
//  The hard-target form (cross entropy) rides in train.hip's row pass (vqf_ce_loss_pred).
//  The order of values -- ties to the lowest index, NaN above +inf -- is common.h's vqf_argmax_key.
#include "common.h"
#include <math.h>

namespace {

constexpr int EV_THREADS = 256;

// this lane's share of the arg-max of x[0..A): 16-byte loads where the row starts on a 16-byte boundary (a maximum does not
// depend on the order it is taken in)
__device__ __forceinline__ unsigned long long row_argmax_key(const float* __restrict__ x, int A) {
  unsigned long long best = 0ull;
  int a0 = 0;
  if (aligned16_dev(x)) {
    const int A4 = A >> 2;
    for (int i = threadIdx.x; i < A4; i += EV_THREADS) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned long long key = vqf_argmax_key(v[e], 4 * i + e);
        best = key > best ? key : best;
      }
    }
    a0 = 4 * A4;
  }
  for (int a = a0 + threadIdx.x; a < A; a += EV_THREADS) {
    const unsigned long long key = vqf_argmax_key(x[a], a);
    best = key > best ? key : best;
  }
  return best;
}

// one block per row n; hit / rowscore: the finish kernel's inputs (workspace)
__global__ __launch_bounds__(EV_THREADS) void match_rows_kernel(const float* __restrict__ logp, const float* __restrict__ target,
                                                                int A, long long* __restrict__ pred,
                                                                long long* __restrict__ tpred, float* __restrict__ score,
                                                                int* __restrict__ hit, float* __restrict__ rowscore) {
  __shared__ unsigned long long shk[4];
  const int n = blockIdx.x;
  const float* t = target + (size_t)n * A;
  const int p = vqf_argmax_index(vqf_block256_max_u64(row_argmax_key(logp + (size_t)n * A, A), shk));
  const int tp = vqf_argmax_index(vqf_block256_max_u64(row_argmax_key(t, A), shk));
  if (threadIdx.x == 0) {
    const float sc = t[p];
    if (pred) pred[n] = p;
    if (tpred) tpred[n] = tp;
    if (score) score[n] = sc;
    hit[n] = (p == tp) ? 1 : 0;
    rowscore[n] = sc;
  }
}

struct MatchTotals {
  long long* counts;     // [0] rows with pred == tpred, [1] rows
  double* score_sum;     // sum of the rows' scores
  const float* loss;     // the batch's criterion value (a device scalar), or NULL
  double* loss_sum;      // += N * loss[0]
  float* acc;            // hits / N of THIS call
  int accumulate;
};

__global__ __launch_bounds__(EV_THREADS) void match_finish_kernel(const int* __restrict__ hit, const float* __restrict__ rowscore,
                                                                  int N, const MatchTotals tt) {
  __shared__ double shd[4];
  __shared__ long long shl[4];
  double ss = 0.0;
  long long hits = 0;
  for (int i = threadIdx.x; i < N; i += EV_THREADS) {
    ss += (double)rowscore[i];
    hits += hit[i];
  }
  ss = vqf_block256_sum(ss, shd);
  hits = vqf_block256_sum(hits, shl);
  if (threadIdx.x == 0) {
    const bool acc = tt.accumulate != 0;
    if (tt.counts) {
      tt.counts[0] = (acc ? tt.counts[0] : 0) + hits;
      tt.counts[1] = (acc ? tt.counts[1] : 0) + N;
    }
    if (tt.score_sum) tt.score_sum[0] = (acc ? tt.score_sum[0] : 0.0) + ss;
    if (tt.loss_sum && tt.loss) tt.loss_sum[0] = (acc ? tt.loss_sum[0] : 0.0) + (double)N * (double)tt.loss[0];
    if (tt.acc) tt.acc[0] = (float)hits / (float)N;
  }
}

// ---- top-k ------------------------------------------------------------------
constexpr int TOPK_HEAD = 64;      // bytes of reduction scratch in front of the row (keeps the row 16-byte aligned in LDS)

// one block per row r; dynamic LDS: TOPK_HEAD + W * 4 bytes
__global__ __launch_bounds__(EV_THREADS) void topk_rows_kernel(const float* __restrict__ x, int ldx, int W, int k, int mode,
                                                               long long* __restrict__ idx, float* __restrict__ val) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* shk = reinterpret_cast<unsigned long long*>(smem);      // 4 words
  float* shf = reinterpret_cast<float*>(smem + 32);                           // 4 floats
  float* row = reinterpret_cast<float*>(smem + TOPK_HEAD);
  const int r = blockIdx.x;
  const float* xr = x + (size_t)r * ldx;
  int a0 = 0;
  if (aligned16_dev(xr)) {           // rows of an odd W (or an odd ldx) start off a 16-byte boundary: those load dword by dword
    const int W4 = W >> 2;
    for (int i = threadIdx.x; i < W4; i += EV_THREADS)
      *reinterpret_cast<f32x4*>(row + 4 * i) = *reinterpret_cast<const f32x4*>(xr + 4 * i);
    a0 = 4 * W4;
  }
  for (int a = a0 + threadIdx.x; a < W; a += EV_THREADS) row[a] = xr[a];
  __syncthreads();

  float mx = 0.f, se = 1.f;
  if (mode == 1) {                   // softmax over the WHOLE row: exp(x - lse) = exp(x - max) / sum exp(x - max)
    mx = -INFINITY;
    for (int a = threadIdx.x; a < W; a += EV_THREADS) mx = fmaxf(mx, row[a]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) shf[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3]));
    se = 0.f;
    for (int a = threadIdx.x; a < W; a += EV_THREADS) se += expf(row[a] - mx);
    se = vqf_block256_sum(se, shf);
  }

  unsigned long long bound = ~0ull;  // above every key
  for (int j = 0; j < k; ++j) {      // k <= W: every round finds an element
    unsigned long long best = 0ull;
    for (int a = threadIdx.x; a < W; a += EV_THREADS) {
      const unsigned long long key = vqf_argmax_key(row[a], a);
      best = (key < bound && key > best) ? key : best;
    }
    bound = vqf_block256_max_u64(best, shk);
    if (threadIdx.x == 0) {
      const int i = vqf_argmax_index(bound);
      const float v = row[i];
      idx[(size_t)r * k + j] = i;
      val[(size_t)r * k + j] = mode == 1 ? expf(v - mx) / se : v;
    }
  }
}

}  // namespace

extern "C" {

int vqf_answer_match_rows(const float* logp, const float* target, int N, int A, long long* pred, long long* tpred,
                          float* score, long long* counts, double* score_sum, const float* loss, double* loss_sum,
                          float* acc, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  if (N <= 0 || A <= 0) return VQF_E_BADARG;
  if (!logp || !target || !ws) return VQF_E_BADARG;
  if (ws_bytes < (size_t)N * (sizeof(int) + sizeof(float))) return VQF_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int* hit = (int*)ws;
  float* rowscore = (float*)(hit + N);
  vqf_prof_dims(N, A, 0);
  VQF_LAUNCH(KID_ANSWER_MATCH, match_rows_kernel, dim3(N), dim3(EV_THREADS), 0, s, logp, target, A, pred, tpred, score, hit,
             rowscore);
  if (counts || score_sum || (loss && loss_sum) || acc)
    hipLaunchKernelGGL(match_finish_kernel, dim3(1), dim3(EV_THREADS), 0, s, (const int*)hit, (const float*)rowscore, N,
                       MatchTotals{counts, score_sum, loss, loss_sum, acc, accumulate});
  return vqf_last_error();
}

int vqf_topk_rows_supported(int W, int k) { return W >= 1 && W <= VQF_TOPK_MAX_W && k >= 1 && k <= VQF_TOPK_MAX_K && k <= W; }

int vqf_topk_rows(const float* x, int R, int W, int ldx, int k, int mode, long long* idx, float* val, void* stream) {
  if (R <= 0 || W <= 0 || k < 1 || k > W || ldx < W) return VQF_E_BADARG;
  if (!x || !idx || !val || (mode != 0 && mode != 1)) return VQF_E_BADARG;
  if (!vqf_topk_rows_supported(W, k)) return VQF_E_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int lds = TOPK_HEAD + W * (int)sizeof(float);      // 16384 floats + the head: just over the 64 KB default
  static VqfDynLdsFlags attr = {};
  if (int e = vqf_set_dyn_lds(reinterpret_cast<const void*>(&topk_rows_kernel), lds, attr)) return e;
  vqf_prof_dims(R, W, k);
  VQF_LAUNCH(KID_TOPK_ROWS, topk_rows_kernel, dim3(R), dim3(EV_THREADS), lds, s, x, ldx, W, k, mode, idx, val);
  return vqf_last_error();
}

}  // extern "C"
