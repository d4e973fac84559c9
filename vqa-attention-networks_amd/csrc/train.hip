// Training-step tail of the solver: the two criteria of solver.py:25-28 with
// their gradients, and torch.optim.Adam (solver.py:29) as one multi-tensor launch.
//
//  * cross entropy (nn.CrossEntropyLoss(), mean over the non-ignored rows, ignore_index = -100):
//    one block per row computes lse, the row loss and dlogits = (softmax - onehot) / count in the
//    same pass; a single-block kernel adds the row losses in a fixed order.  vqf_ce_loss_pred is the same two launches
//    with the solver's next lines (solver.py:96-101) riding in them: the row's arg-max, the hit count, the loss total.
//  * KL divergence (nn.KLDivLoss(), default reduction: mean over all N*A elements):
//    loss = mean(t * (log t - logp)) with 0 where t == 0; dlogp = -t / (N*A).
//  * binary cross entropy with logits on soft answers (vqa_amd.BCEWithLogitsLoss; not in the reference, whose solver asserts
//    hard labels for the models that return logits): one block per row, one read of the row -- row loss, dlogits, the row's
//    arg-max and the soft score of the predicted answer; the target dense (N,A) or K sparse (id, score) slots per row.
//  * Adam: m, v, p updated in place in the order of torch's single-tensor path; HBM-bound
//    (16 B read + 12 B written per element).  Adamax (torch.optim.Adamax; not in the reference) is the same kernel template.
//  * gradient-norm clipping (torch.nn.utils.clip_grad_norm_, norm_type 2; not in the reference): a multi-tensor sum of squares
//    (4 B read per element, one partial per block, no atomics), a single-block finish in double that leaves the norm and the
//    clip coefficient on the device, an in-place multi-tensor scale -- or the optimizer kernel reading the coefficient itself.
#include "common.h"
#include <math.h>

namespace {

constexpr int TR_THREADS = 256;

// one block per row n.  PRED: the row's argmax rides in the pass that finds the maximum for the log-sum-exp, as one
// (value, index) key per lane (vqf_argmax_key: ties to the lowest index, NaN above everything); loss and dlogits keep the
// arithmetic and the reduction order of the plain form, so both instantiations give the same bits.
template <bool PRED>
__global__ __launch_bounds__(TR_THREADS) void ce_rows_kernel(const float* __restrict__ logits,
                                                             const long long* __restrict__ target, int N, int A,
                                                             float* __restrict__ rowloss,
                                                             float* __restrict__ dlogits,
                                                             long long* __restrict__ pred, int* __restrict__ hit) {
  __shared__ float sh[4];
  __shared__ unsigned long long shk[4];
  const int n = blockIdx.x;
  // rows that count (every block recomputes it: N int64 loads out of L2)
  float cnt = 0.f;
  for (int i = threadIdx.x; i < N; i += TR_THREADS) cnt += (target[i] != -100) ? 1.f : 0.f;
  cnt = vqf_block256_sum(cnt, sh);
  const float inv_cnt = cnt > 0.f ? 1.f / cnt : 0.f;

  const float* x = logits + (size_t)n * A;
  float mx = -INFINITY;
  unsigned long long best = 0ull;
  for (int a = threadIdx.x; a < A; a += TR_THREADS) {
    const float v = x[a];
    mx = fmaxf(mx, v);
    if (PRED) {
      const unsigned long long key = vqf_argmax_key(v, a);
      best = key > best ? key : best;
    }
  }
  mx = vqf_block256_max(mx, sh);
  float se = 0.f;
  for (int a = threadIdx.x; a < A; a += TR_THREADS) se += expf(x[a] - mx);
  se = vqf_block256_sum(se, sh);
  const float lse = mx + logf(se);
  const long long t = target[n];
  const bool live = (t != -100);
  if (threadIdx.x == 0) rowloss[n] = (live && t >= 0 && t < A) ? (lse - x[t]) : (live ? NAN : 0.f);
  if (PRED) {
    const int p = vqf_argmax_index(vqf_block256_max_u64(best, shk));
    if (threadIdx.x == 0) {
      if (pred) pred[n] = p;
      hit[n] = (live && (long long)p == t) ? 1 : 0;      // an out-of-range target is never a hit
    }
  }
  if (dlogits) {
    float* d = dlogits + (size_t)n * A;
    const float inv_se = 1.f / se;
    for (int a = threadIdx.x; a < A; a += TR_THREADS) {
      float p = expf(x[a] - mx) * inv_se;
      d[a] = live ? (p - ((long long)a == t ? 1.f : 0.f)) * inv_cnt : 0.f;
    }
  }
}

// what the evaluation tail adds to the finish (vqf_ce_loss_pred): hit[N] per-row flags of the row kernel; every output may be NULL
struct LossTotals {
  const int* hit;
  long long* counts;     // [0] hits, [1] rows whose target != -100
  double* loss_sum;      // sum of the row losses (ignored rows hold 0)
  float* acc;            // hits / counted rows of THIS call
  int accumulate;        // != 0: counts and loss_sum are added to
};

// loss = sum(part[0..P)) * scale  (scale < 0: divide by the number of targets != -100 instead)
template <bool TOTALS>
__global__ __launch_bounds__(TR_THREADS) void loss_finish_kernel(const float* __restrict__ part, int P, float scale,
                                                                 const long long* __restrict__ target, int N,
                                                                 float* __restrict__ loss, const LossTotals tt) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < P; i += TR_THREADS) s += part[i];
  s = vqf_block256_sum(s, sh);
  if (target) {
    float cnt = 0.f;
    for (int i = threadIdx.x; i < N; i += TR_THREADS) cnt += (target[i] != -100) ? 1.f : 0.f;
    cnt = vqf_block256_sum(cnt, sh);
    scale = 1.f / cnt;       // 0/0 -> NaN like torch when every row is ignored
  }
  if (threadIdx.x == 0) loss[0] = s * scale;
  if (TOTALS) {              // P == N row losses, target != NULL; the same fixed order as above, in double / integers
    __shared__ double shd[4];
    __shared__ long long shl[4];
    double ds = 0.0;
    long long hits = 0, rows = 0;
    for (int i = threadIdx.x; i < N; i += TR_THREADS) {
      ds += (double)part[i];
      hits += tt.hit[i];
      rows += (target[i] != -100) ? 1 : 0;
    }
    ds = vqf_block256_sum(ds, shd);
    hits = vqf_block256_sum(hits, shl);
    rows = vqf_block256_sum(rows, shl);
    if (threadIdx.x == 0) {
      if (tt.counts) {
        tt.counts[0] = (tt.accumulate ? tt.counts[0] : 0) + hits;
        tt.counts[1] = (tt.accumulate ? tt.counts[1] : 0) + rows;
      }
      if (tt.loss_sum) tt.loss_sum[0] = (tt.accumulate ? tt.loss_sum[0] : 0.0) + ds;
      if (tt.acc) tt.acc[0] = (float)hits / (float)rows;      // 0 / 0 = NaN: the mean of no rows
    }
  }
}

// ---- BCE with logits on soft answers (vqf_bce_loss / vqf_bce_loss_sparse) -----------------------------------------------
// sigma(x) from e = exp(-|x|) in (0, 1]: no overflow on either sign
__device__ __forceinline__ float bce_sigmoid(float x, float e) {
  const float r = 1.f / (1.f + e);
  return x >= 0.f ? r : e * r;
}
// the soft targets of a row as K (id, score) slots; a slot whose id is outside [0, A) is empty and its score is never used
struct BceSlots {
  const void* ids;       // (N, K) int32 or int64
  const float* scores;   // (N, K)
  int K, ids64;
};
__device__ __forceinline__ long long bce_slot_id(const BceSlots& sl, size_t i) {
  return sl.ids64 ? ((const long long*)sl.ids)[i] : (long long)((const int*)sl.ids)[i];
}

// one block per row n, one read of the row: the row loss sum_a [max(x,0) - x t + log1p(exp(-|x|))], dlogits = (sigma(x) - t) c,
// the arg-max (the key of ce_rows_kernel<true>) and score = t[pred].  SPARSE: the pass runs on a zero target; the live slots then
// subtract s_k x[id_k] from the row loss (thread 0, slot order) and, after a workgroup barrier, the first slot of each live id
// rewrites ITS element as (sigma(x) - t) c with t = the sum of that id's scores in slot order: the expression of the dense form,
// so distinct ids give the dense gradient's bits.  Every such store lands inside row n (0 <= id < A), made by this workgroup.
template <bool SPARSE>
__global__ __launch_bounds__(TR_THREADS) void bce_rows_kernel(const float* __restrict__ logits,
                                                              const float* __restrict__ target, const BceSlots sl, int A,
                                                              float c, float* __restrict__ rowloss,
                                                              float* __restrict__ rowscore, float* __restrict__ dlogits,
                                                              long long* __restrict__ pred, float* __restrict__ score) {
  __shared__ float sh[4];
  __shared__ unsigned long long shk[4];
  const int n = blockIdx.x;
  const float* x = logits + (size_t)n * A;
  const float* t = SPARSE ? nullptr : target + (size_t)n * A;
  float* d = dlogits ? dlogits + (size_t)n * A : nullptr;
  float s = 0.f;
  unsigned long long best = 0ull;
  for (int a = threadIdx.x; a < A; a += TR_THREADS) {
    const float v = x[a];
    const float e = expf(-fabsf(v));
    const float ta = SPARSE ? 0.f : t[a];
    s += (fmaxf(v, 0.f) - v * ta) + log1pf(e);
    const unsigned long long key = vqf_argmax_key(v, a);
    best = key > best ? key : best;
    if (d) d[a] = (bce_sigmoid(v, e) - ta) * c;
  }
  s = vqf_block256_sum(s, sh);
  const int p = vqf_argmax_index(vqf_block256_max_u64(best, shk));
  const size_t k0 = (size_t)n * (SPARSE ? sl.K : 0);
  if (threadIdx.x == 0) {
    float sc = 0.f;
    if (SPARSE) {
      float corr = 0.f;
      for (int k = 0; k < sl.K; ++k) {
        const long long id = bce_slot_id(sl, k0 + k);
        if (id >= 0 && id < A) {
          const float sk = sl.scores[k0 + k];
          corr += sk * x[id];
          if (id == p) sc += sk;
        }
      }
      s -= corr;
    } else {
      sc = t[p];
    }
    rowloss[n] = s;
    rowscore[n] = sc;
    if (pred) pred[n] = p;
    if (score) score[n] = sc;
  }
  if (SPARSE && d) {
    __syncthreads();       // the row's sigma(x) c stores above are complete before a slot's element is rewritten
    const int k = threadIdx.x;
    if (k < sl.K) {
      const long long id = bce_slot_id(sl, k0 + k);
      if (id >= 0 && id < A) {
        bool first = true;
        float tk = 0.f;
        for (int j = 0; j < sl.K; ++j) {
          if (bce_slot_id(sl, k0 + j) == id) {
            first = first && j >= k;
            tk += sl.scores[k0 + j];
          }
        }
        if (first) {
          const float v = x[id];
          d[id] = (bce_sigmoid(v, expf(-fabsf(v))) - tk) * c;
        }
      }
    }
  }
}

struct BceTotals {
  long long* rows;       // [0] the rows of the call(s)
  double* score_sum;     // sum of the rows' scores
  double* loss_sum;      // N * loss, from the double row sum
  float* acc;            // the mean score of THIS call
  int accumulate;        // != 0: rows, score_sum and loss_sum are added to
};

// loss = c * sum(rowloss[0..N)) in the fixed order of loss_finish_kernel; the totals in double; every total may be NULL
__global__ __launch_bounds__(TR_THREADS) void bce_finish_kernel(const float* __restrict__ rowloss,
                                                                const float* __restrict__ rowscore, int N, float c,
                                                                double row_weight, float* __restrict__ loss,
                                                                const BceTotals tt) {
  __shared__ float sh[4];
  __shared__ double shd[4];
  float s = 0.f;
  double ds = 0.0, ss = 0.0;
  for (int i = threadIdx.x; i < N; i += TR_THREADS) {
    s += rowloss[i];
    ds += (double)rowloss[i];
    ss += (double)rowscore[i];
  }
  s = vqf_block256_sum(s, sh);
  ds = vqf_block256_sum(ds, shd);
  ss = vqf_block256_sum(ss, shd);
  if (threadIdx.x == 0) {
    const bool acc = tt.accumulate != 0;
    loss[0] = s * c;
    if (tt.rows) tt.rows[0] = (acc ? tt.rows[0] : 0) + N;
    if (tt.score_sum) tt.score_sum[0] = (acc ? tt.score_sum[0] : 0.0) + ss;
    if (tt.loss_sum) tt.loss_sum[0] = (acc ? tt.loss_sum[0] : 0.0) + row_weight * ds;     // row_weight = N * c
    if (tt.acc) tt.acc[0] = (float)(ss / (double)N);
  }
}

// element-wise part of KLDivLoss; each block reduces a contiguous chunk into part[blockIdx.x]
constexpr int KL_PER_BLOCK = TR_THREADS * 16;
__global__ __launch_bounds__(TR_THREADS) void kldiv_kernel(const float* __restrict__ logp,
                                                           const float* __restrict__ tgt, long long n, float inv_n,
                                                           float* __restrict__ part, float* __restrict__ dlogp) {
  __shared__ float sh[4];
  const long long base = (long long)blockIdx.x * KL_PER_BLOCK;
  float s = 0.f;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    long long i = base + j * TR_THREADS + threadIdx.x;
    if (i < n) {
      float t = tgt[i], x = logp[i];
      s += t > 0.f ? t * (logf(t) - x) : (t == 0.f ? 0.f : NAN);
      if (dlogp) dlogp[i] = -t * inv_n;
    }
  }
  s = vqf_block256_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- Adam / Adamax, gradient-norm clipping ------------------------------------
constexpr int ADAM_MAX_TENSORS = VQF_ADAM_MAX_TENSORS;
constexpr int ADAM_CHUNK = TR_THREADS * 16;      // elements per block
struct AdamTable {
  float* p[ADAM_MAX_TENSORS];
  const float* g[ADAM_MAX_TENSORS];
  float* m[ADAM_MAX_TENSORS];
  float* v[ADAM_MAX_TENSORS];
  long long n[ADAM_MAX_TENSORS];
  int block0[ADAM_MAX_TENSORS + 1];   // first block of tensor i
  int count;
};
// Adamax reads beta2, one_m_beta1, eps, wd and step_size (= clr = lr / (1 - beta1^step)); v holds exp_inf
struct AdamHyper { float beta1, beta2, one_m_beta1, one_m_beta2, eps, wd, step_size, bc2_sqrt; };
constexpr int RULE_ADAM = 0, RULE_ADAMAX = 1;

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamHyper& h) {
  if (h.wd != 0.f) g = g + h.wd * p;
  m = m + (g - m) * h.one_m_beta1;                 // exp_avg.lerp_(grad, 1 - beta1)
  v = v * h.beta2 + h.one_m_beta2 * g * g;         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = p - h.step_size * (m / denom);               // param.addcdiv_(exp_avg, denom, -step_size)
}
__device__ __forceinline__ void adamax_one(float& p, float g, float& m, float& u, const AdamHyper& h) {
  if (h.wd != 0.f) g = g + h.wd * p;
  m = m + (g - m) * h.one_m_beta1;                 // exp_avg.lerp_(grad, 1 - beta1)
  const float a = u * h.beta2, b = fabsf(g) + h.eps;
  u = (b > a || b != b) ? b : a;                   // torch.maximum(exp_inf.mul_(beta2), grad.abs().add_(eps)): NaN on either side stays
  p = p - h.step_size * (m / u);                   // param.addcdiv_(exp_avg, exp_inf, -clr)
}
template <int RULE>
__device__ __forceinline__ void optim_one(float& p, float g, float& m, float& v, const AdamHyper& h) {
  if (RULE == RULE_ADAMAX) adamax_one(p, g, m, v, h); else adam_one(p, g, m, v, h);
}

// SCALED: the gradient the update sees is g * *grad_scale (one fp32 rounding, before weight decay; the clip coefficient of
// grad_norm_finish_kernel, loaded once per block); the gradient in memory is not written.
// Scale: empty (vqf_adam_step's kernel is <RULE_ADAM>, under the kernel arguments it has always had), or one const float*.
template <int RULE, typename... Scale>
__global__ __launch_bounds__(TR_THREADS) void adam_kernel(const AdamTable tb, const AdamHyper h, Scale... grad_scale) {
  constexpr bool SCALED = sizeof...(Scale) != 0;
  // block -> tensor (uniform scan of <= 32 entries held in kernarg SGPRs)
  int ti = 0;
  const int b = blockIdx.x;
  while (ti + 1 < tb.count && b >= tb.block0[ti + 1]) ++ti;
  float* __restrict__ p = tb.p[ti];
  const float* __restrict__ g = tb.g[ti];
  float* __restrict__ m = tb.m[ti];
  float* __restrict__ v = tb.v[ti];
  const long long n = tb.n[ti];
  const long long base = (long long)(b - tb.block0[ti]) * ADAM_CHUNK;
  const bool vec = aligned16_dev(p) && aligned16_dev(g) && aligned16_dev(m) && aligned16_dev(v);
  float gs = 1.f;
  if constexpr (SCALED) gs = *(grad_scale, ...);
  if (vec && base + ADAM_CHUNK <= n) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      long long i = base + (long long)(j * TR_THREADS + threadIdx.x) * 4;
      f32x4 pp = *(const f32x4*)(p + i), gg = *(const f32x4*)(g + i);
      f32x4 mm = *(const f32x4*)(m + i), vv = *(const f32x4*)(v + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pp[e], me = mm[e], ve = vv[e];
        float ge = gg[e];
        if constexpr (SCALED) ge = ge * gs;
        optim_one<RULE>(pe, ge, me, ve, h);
        pp[e] = pe; mm[e] = me; vv[e] = ve;
      }
      *(f32x4*)(p + i) = pp; *(f32x4*)(m + i) = mm; *(f32x4*)(v + i) = vv;
    }
  } else {
    for (int j = 0; j < 16; ++j) {
      long long i = base + j * TR_THREADS + threadIdx.x;
      if (i < n) {
        float pp = p[i], mm = m[i], vv = v[i];
        float ge = g[i];
        if constexpr (SCALED) ge = ge * gs;
        optim_one<RULE>(pp, ge, mm, vv, h);
        p[i] = pp; m[i] = mm; v[i] = vv;
      }
    }
  }
}

// The gradients of a launch of the norm / scale passes: the block -> tensor mapping of adam_kernel.
struct GradTable {
  float* g[ADAM_MAX_TENSORS];
  long long n[ADAM_MAX_TENSORS];
  int block0[ADAM_MAX_TENSORS + 1];
  int count;
};

// part[blockIdx.x] = the sum of the squares of this block's ADAM_CHUNK elements: 16 squares and adds per thread in index order
// (either path), the wave butterfly, the four wave sums in order.  No atomics: the same memory gives the same bits.
__global__ __launch_bounds__(TR_THREADS) void grad_sumsq_kernel(const GradTable tb, float* __restrict__ part) {
  __shared__ float sh[4];
  int ti = 0;
  const int b = blockIdx.x;
  while (ti + 1 < tb.count && b >= tb.block0[ti + 1]) ++ti;
  const float* __restrict__ g = tb.g[ti];
  const long long n = tb.n[ti];
  const long long base = (long long)(b - tb.block0[ti]) * ADAM_CHUNK;
  float s = 0.f;
  if (aligned16_dev(g) && base + ADAM_CHUNK <= n) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long i = base + (long long)(j * TR_THREADS + threadIdx.x) * 4;
      const f32x4 x = *(const f32x4*)(g + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += x[e] * x[e];
    }
  } else {
    for (int j = 0; j < 16; ++j) {
      const long long i = base + j * TR_THREADS + threadIdx.x;
      if (i < n) {
        const float x = g[i];
        s += x * x;
      }
    }
  }
  s = vqf_block256_sum(s, sh);
  if (threadIdx.x == 0) part[b] = s;
}

// one workgroup: norm = (float)sqrt(sum of part[0..P) in double, fixed order), coef = min(1, max_norm / (norm + 1e-6)) in fp32 as
// torch.nn.utils.clip_grad_norm_ forms it -- `max_norm / tensor` is tensor.reciprocal() * max_norm, then clamp(max = 1), which
// keeps a NaN (norm NaN -> coef NaN) and turns norm = Inf into 0
__global__ __launch_bounds__(TR_THREADS) void grad_norm_finish_kernel(const float* __restrict__ part, long long P,
                                                                      float max_norm, float* __restrict__ norm,
                                                                      float* __restrict__ coef) {
  __shared__ double shd[4];
  double s = 0.0;
  long long i = threadIdx.x;
  for (; i + 7LL * TR_THREADS < P; i += 8LL * TR_THREADS) {      // eight loads in flight (the pass is latency-bound), added in index order
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = part[i + (long long)k * TR_THREADS];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += (double)x[k];
  }
  for (; i < P; i += TR_THREADS) s += (double)part[i];
  s = vqf_block256_sum(s, shd);
  if (threadIdx.x == 0) {
    const float nm = (float)sqrt(s);
    float c = (1.0f / (nm + 1e-6f)) * max_norm;
    if (c > 1.0f) c = 1.0f;
    norm[0] = nm;
    coef[0] = c;
  }
}

// g *= *scale, one fp32 multiply per element
__global__ __launch_bounds__(TR_THREADS) void grad_scale_kernel(const GradTable tb, const float* __restrict__ scale) {
  int ti = 0;
  const int b = blockIdx.x;
  while (ti + 1 < tb.count && b >= tb.block0[ti + 1]) ++ti;
  float* __restrict__ g = tb.g[ti];
  const long long n = tb.n[ti];
  const long long base = (long long)(b - tb.block0[ti]) * ADAM_CHUNK;
  const float c = *scale;
  if (aligned16_dev(g) && base + ADAM_CHUNK <= n) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long i = base + (long long)(j * TR_THREADS + threadIdx.x) * 4;
      f32x4 x = *(const f32x4*)(g + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = x[e] * c;
      *(f32x4*)(g + i) = x;
    }
  } else {
    for (int j = 0; j < 16; ++j) {
      const long long i = base + j * TR_THREADS + threadIdx.x;
      if (i < n) g[i] = g[i] * c;
    }
  }
}

// The next launch's worth of `tensors` from index i on: up to ADAM_MAX_TENSORS non-empty entries whose blocks fit one grid.
// ALL: every pointer of a descriptor is needed (the optimizer steps); otherwise grad and n only.  Returns VQF_OK with
// tb.count == 0 when nothing is left.
template <typename Table, typename Put>
int next_table(const VqfAdamTensor* tensors, int count, int& i, bool all, Table& tb, long long& blocks, Put put) {
  tb.count = 0;
  blocks = 0;
  while (i < count && tb.count < ADAM_MAX_TENSORS) {
    const VqfAdamTensor& t = tensors[i];
    if (t.n < 0) return VQF_E_BADARG;
    if (t.n == 0) { ++i; continue; }
    if (!t.grad || (all && (!t.param || !t.exp_avg || !t.exp_avg_sq))) return VQF_E_BADARG;
    const long long nb = (t.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
    if (blocks + nb > 0x7fffffffLL) break;
    const int k = tb.count++;
    put(k, &t);
    tb.n[k] = t.n;
    tb.block0[k] = (int)blocks;
    blocks += nb;
    ++i;
  }
  if (tb.count == 0) return i < count ? VQF_E_UNSUPPORTED : VQF_OK;   // a single tensor too large for one grid
  tb.block0[tb.count] = (int)blocks;
  for (int k = tb.count; k < ADAM_MAX_TENSORS; ++k) {
    put(k, nullptr);
    tb.n[k] = 0;
    tb.block0[k + 1] = (int)blocks;
  }
  return VQF_OK;
}

int optim_step(int rule, const VqfAdamTensor* tensors, int count, const AdamHyper& h, const float* grad_scale,
               hipStream_t s) {
  int i = 0;
  while (i < count) {
    AdamTable tb;
    long long blocks = 0;
    const int st = next_table(tensors, count, i, true, tb, blocks, [&](int k, const VqfAdamTensor* t) {
      tb.p[k] = t ? t->param : nullptr; tb.g[k] = t ? t->grad : nullptr;
      tb.m[k] = t ? t->exp_avg : nullptr; tb.v[k] = t ? t->exp_avg_sq : nullptr;
    });
    if (st) return st;
    if (tb.count == 0) break;
    vqf_prof_dims(tb.count, (int)(blocks > 0x7fffffff ? 0x7fffffff : blocks), 0);
    const dim3 grid((unsigned)blocks), block(TR_THREADS);
    if (rule == RULE_ADAMAX) {
      if (grad_scale) VQF_LAUNCH(KID_ADAMAX, (adam_kernel<RULE_ADAMAX, const float*>), grid, block, 0, s, tb, h, grad_scale);
      else VQF_LAUNCH(KID_ADAMAX, adam_kernel<RULE_ADAMAX>, grid, block, 0, s, tb, h);
    } else {
      if (grad_scale) VQF_LAUNCH(KID_ADAM_SCALED, (adam_kernel<RULE_ADAM, const float*>), grid, block, 0, s, tb, h, grad_scale);
      else VQF_LAUNCH(KID_ADAM, adam_kernel<RULE_ADAM>, grid, block, 0, s, tb, h);
    }
    const int rc = vqf_last_error();
    if (rc) return rc;
  }
  return VQF_OK;
}

// the blocks (= partials) of all of `tensors`, or -1 for a negative size
long long grad_blocks(const VqfAdamTensor* tensors, int count) {
  long long blocks = 0;
  for (int i = 0; i < count; ++i) {
    if (tensors[i].n < 0) return -1;
    blocks += (tensors[i].n + ADAM_CHUNK - 1) / ADAM_CHUNK;
  }
  return blocks;
}
bool aligned4(const void* p) { return (((uintptr_t)p) & 3) == 0; }

}  // namespace

extern "C" {

size_t vqf_loss_ws_bytes(int N, int A) {
  long long n = (long long)N * A;
  long long parts = (n + KL_PER_BLOCK - 1) / KL_PER_BLOCK;
  if (parts < N) parts = N;
  return (size_t)(parts > 0 ? parts : 1) * sizeof(float);
}

int vqf_ce_loss(const float* logits, const long long* target, int N, int A, float* loss, float* dlogits,
                void* ws, size_t ws_bytes, void* stream) {
  if (N <= 0 || A <= 0) return VQF_E_BADARG;
  if (!logits || !target || !loss || !ws) return VQF_E_BADARG;
  if (ws_bytes < (size_t)N * sizeof(float)) return VQF_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* rowloss = (float*)ws;
  vqf_prof_dims(N, A, 0);
  VQF_LAUNCH(KID_CE_LOSS, ce_rows_kernel<false>, dim3(N), dim3(TR_THREADS), 0, s, logits, target, N, A, rowloss, dlogits,
             (long long*)nullptr, (int*)nullptr);
  hipLaunchKernelGGL(loss_finish_kernel<false>, dim3(1), dim3(TR_THREADS), 0, s, (const float*)rowloss, N, -1.f, target, N,
                     loss, LossTotals{});
  return vqf_last_error();
}

int vqf_ce_loss_pred(const float* logits, const long long* target, int N, int A, float* loss, float* dlogits,
                     long long* pred, long long* counts, double* loss_sum, float* acc, int accumulate, void* ws,
                     size_t ws_bytes, void* stream) {
  if (N <= 0 || A <= 0) return VQF_E_BADARG;
  if (!logits || !target || !loss || !ws) return VQF_E_BADARG;
  if (ws_bytes < (size_t)N * (sizeof(float) + sizeof(int))) return VQF_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* rowloss = (float*)ws;
  int* hit = (int*)(rowloss + N);
  vqf_prof_dims(N, A, 0);
  VQF_LAUNCH(KID_CE_LOSS_PRED, ce_rows_kernel<true>, dim3(N), dim3(TR_THREADS), 0, s, logits, target, N, A, rowloss,
             dlogits, pred, hit);
  hipLaunchKernelGGL(loss_finish_kernel<true>, dim3(1), dim3(TR_THREADS), 0, s, (const float*)rowloss, N, -1.f, target, N,
                     loss, LossTotals{hit, counts, loss_sum, acc, accumulate});
  return vqf_last_error();
}

int vqf_kldiv_loss(const float* logp, const float* target, int N, int A, float* loss, float* dlogp, void* ws,
                   size_t ws_bytes, void* stream) {
  if (N <= 0 || A <= 0) return VQF_E_BADARG;
  if (!logp || !target || !loss || !ws) return VQF_E_BADARG;
  const long long n = (long long)N * A;
  const long long parts = (n + KL_PER_BLOCK - 1) / KL_PER_BLOCK;
  if (parts > 0x7fffffffLL) return VQF_E_BADARG;
  if (ws_bytes < (size_t)parts * sizeof(float)) return VQF_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  const float inv_n = (float)(1.0 / (double)n);
  vqf_prof_dims(N, A, 0);
  VQF_LAUNCH(KID_KLDIV_LOSS, kldiv_kernel, dim3((unsigned)parts), dim3(TR_THREADS), 0, s, logp, target, n, inv_n, part,
             dlogp);
  hipLaunchKernelGGL(loss_finish_kernel<false>, dim3(1), dim3(TR_THREADS), 0, s, (const float*)part, (int)parts, inv_n,
                     (const long long*)nullptr, 0, loss, LossTotals{});
  return vqf_last_error();
}

size_t vqf_bce_loss_ws_bytes(int N) { return N > 0 ? (size_t)N * 2 * sizeof(float) : 0; }

static int bce_loss_launch(bool sparse, const float* logits, const float* target, const BceSlots& sl, int N, int A,
                           double scale, float* loss, float* dlogits, long long* pred, float* score, long long* rows,
                           double* score_sum, double* loss_sum, float* acc, int accumulate, void* ws, size_t ws_bytes,
                           void* stream) {
  if (N <= 0 || A <= 0) return VQF_E_BADARG;
  if (sparse ? (!sl.ids || !sl.scores || sl.K < 1 || sl.K > VQF_SOFT_MAX_SLOTS) : !target) return VQF_E_BADARG;
  if (!logits || !loss || !ws) return VQF_E_BADARG;
  if (ws_bytes < vqf_bce_loss_ws_bytes(N)) return VQF_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* rowloss = (float*)ws;
  float* rowscore = rowloss + N;
  const float c = (float)scale;
  vqf_prof_dims(N, A, sparse ? sl.K : 0);
  if (sparse)
    VQF_LAUNCH(KID_BCE_LOSS_SPARSE, bce_rows_kernel<true>, dim3(N), dim3(TR_THREADS), 0, s, logits, target, sl, A, c, rowloss,
               rowscore, dlogits, pred, score);
  else
    VQF_LAUNCH(KID_BCE_LOSS, bce_rows_kernel<false>, dim3(N), dim3(TR_THREADS), 0, s, logits, target, sl, A, c, rowloss,
               rowscore, dlogits, pred, score);
  hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(TR_THREADS), 0, s, (const float*)rowloss, (const float*)rowscore, N, c,
                     (double)N * scale, loss, BceTotals{rows, score_sum, loss_sum, acc, accumulate});
  return vqf_last_error();
}

int vqf_bce_loss(const float* logits, const float* target, int N, int A, double scale, float* loss, float* dlogits,
                 long long* pred, float* score, long long* rows, double* score_sum, double* loss_sum, float* acc,
                 int accumulate, void* ws, size_t ws_bytes, void* stream) {
  return bce_loss_launch(false, logits, target, BceSlots{nullptr, nullptr, 0, 0}, N, A, scale, loss, dlogits, pred, score, rows,
                         score_sum, loss_sum, acc, accumulate, ws, ws_bytes, stream);
}

int vqf_bce_loss_sparse(const float* logits, const void* ids, int ids64, const float* scores, int K, int N, int A,
                        double scale, float* loss, float* dlogits, long long* pred, float* score, long long* rows,
                        double* score_sum, double* loss_sum, float* acc, int accumulate, void* ws, size_t ws_bytes,
                        void* stream) {
  return bce_loss_launch(true, logits, nullptr, BceSlots{ids, scores, K, ids64 != 0}, N, A, scale, loss, dlogits, pred, score,
                         rows, score_sum, loss_sum, acc, accumulate, ws, ws_bytes, stream);
}

static void adam_hyper(double lr, double beta1, double beta2, double eps, double weight_decay, long long step, AdamHyper& h) {
  // hyper-parameters are combined in double and rounded once, as torch does with its Python scalars
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  h.beta1 = (float)beta1; h.beta2 = (float)beta2;
  h.one_m_beta1 = (float)(1.0 - beta1); h.one_m_beta2 = (float)(1.0 - beta2);
  h.eps = (float)eps; h.wd = (float)weight_decay;
  h.step_size = (float)(lr / bc1);
  h.bc2_sqrt = (float)sqrt(bc2);
}

int vqf_adam_step(const VqfAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                  double weight_decay, long long step, void* stream) {
  if (count < 0 || step < 1) return VQF_E_BADARG;
  if (count && !tensors) return VQF_E_BADARG;
  AdamHyper h;
  adam_hyper(lr, beta1, beta2, eps, weight_decay, step, h);
  return optim_step(RULE_ADAM, tensors, count, h, nullptr, (hipStream_t)stream);
}

int vqf_adam_step_scaled(const VqfAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                         double weight_decay, long long step, const float* grad_scale, void* stream) {
  if (count < 0 || step < 1) return VQF_E_BADARG;
  if ((count && !tensors) || !grad_scale) return VQF_E_BADARG;
  if (!aligned4(grad_scale)) return VQF_E_ALIGN;
  AdamHyper h;
  adam_hyper(lr, beta1, beta2, eps, weight_decay, step, h);
  return optim_step(RULE_ADAM, tensors, count, h, grad_scale, (hipStream_t)stream);
}

int vqf_adamax_step(const VqfAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                    double weight_decay, long long step, const float* grad_scale, void* stream) {
  if (count < 0 || step < 1) return VQF_E_BADARG;
  if (count && !tensors) return VQF_E_BADARG;
  if (!aligned4(grad_scale)) return VQF_E_ALIGN;
  AdamHyper h;
  adam_hyper(lr, beta1, beta2, eps, weight_decay, step, h);      // step_size = clr = lr / (1 - beta1^step)
  return optim_step(RULE_ADAMAX, tensors, count, h, grad_scale, (hipStream_t)stream);
}

size_t vqf_grad_norm_ws_bytes(const VqfAdamTensor* tensors, int count) {
  if (count <= 0 || !tensors) return 0;
  const long long blocks = grad_blocks(tensors, count);
  return blocks > 0 ? (size_t)blocks * sizeof(float) : 0;
}

int vqf_grad_norm_clip(const VqfAdamTensor* tensors, int count, double max_norm, float* norm, float* coef, void* ws,
                       size_t ws_bytes, void* stream) {
  if (count < 0 || (count && !tensors) || !norm || !coef) return VQF_E_BADARG;
  if (!(max_norm > 0.0)) return VQF_E_BADARG;                    // (a NaN is refused as well)
  const long long total = grad_blocks(tensors, count);
  if (total < 0) return VQF_E_BADARG;
  for (int i = 0; i < count; ++i)
    if (tensors[i].n > 0 && !tensors[i].grad) return VQF_E_BADARG;
  if (total > 0 && !ws) return VQF_E_BADARG;
  if (ws_bytes < (size_t)total * sizeof(float)) return VQF_E_WORKSPACE;
  if (!aligned4(norm) || !aligned4(coef) || !aligned4(ws)) return VQF_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  long long done = 0;
  int i = 0;
  while (i < count) {
    GradTable tb;
    long long blocks = 0;
    const int st = next_table(tensors, count, i, false, tb, blocks,
                              [&](int k, const VqfAdamTensor* t) { tb.g[k] = t ? const_cast<float*>(t->grad) : nullptr; });
    if (st) return st;
    if (tb.count == 0) break;
    vqf_prof_dims(tb.count, (int)blocks, 0);
    VQF_LAUNCH(KID_GRAD_SUMSQ, grad_sumsq_kernel, dim3((unsigned)blocks), dim3(TR_THREADS), 0, s, tb, part + done);
    const int rc = vqf_last_error();
    if (rc) return rc;
    done += blocks;
  }
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(TR_THREADS), 0, s, (const float*)part, done, (float)max_norm, norm,
                     coef);
  return vqf_last_error();
}

int vqf_grad_scale(const VqfAdamTensor* tensors, int count, const float* scale, void* stream) {
  if (count < 0 || (count && !tensors) || !scale) return VQF_E_BADARG;
  if (!aligned4(scale)) return VQF_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  int i = 0;
  while (i < count) {
    GradTable tb;
    long long blocks = 0;
    const int st = next_table(tensors, count, i, false, tb, blocks,
                              [&](int k, const VqfAdamTensor* t) { tb.g[k] = t ? const_cast<float*>(t->grad) : nullptr; });
    if (st) return st;
    if (tb.count == 0) break;
    vqf_prof_dims(tb.count, (int)blocks, 0);
    VQF_LAUNCH(KID_GRAD_SCALE, grad_scale_kernel, dim3((unsigned)blocks), dim3(TR_THREADS), 0, s, tb, scale);
    const int rc = vqf_last_error();
    if (rc) return rc;
  }
  return VQF_OK;
}

}  // extern "C"
