// Guided attention logits: the streaming passes of HieCoAttenLadder's ALTERNATING co-attention (host/hie_ladder.py,
// coatt="alternating"; Lu et al. 2016, section 3.3).  One attention step is
//   Xh = X Wx^T + bx   (a GEMM, (N*S, E))          H = tanh(Xh + gp[n])   with the per-sample guidance row gp[n] = g[n] Wg^T
//   logit[n, s] = H[n, s, :] . w                    a = softmax_S(logit), x^ = sum_s a[s] X[s]   (vqf_glimpse_pool_*)
// and the two kernels here are the H line and its backward for G <= 3 steps that share the rows (the three levels' image
// attention: Xh (N*S, ldx) with step g's block at columns [g E, (g + 1) E), gp (N, G E), w (G, E)).  H is never stored:
//   fwd   logits[r, g] = sum_e w[g, e] tanh(Xh[r, g E + e] + gp[n, g E + e])                 one read of Xh, (N*S, G) out
//   bwd   recomputes H;  dXh[r, g, e] = dlogits[r, g] w[g, e] (1 - H^2)                      one read of Xh, one write of dXh
//         dgp[n, :] = sum_s dXh[n, s, :]     dw[g, e] = sum_{n, s} dlogits[n, s, g] H[n, s, g, e]
// gp = null is the unguided step (H = tanh(Xh)): the guidance row is taken as zeros, x + 0 == x, the same kernel.
// Both are HBM streams.  A workgroup's rows belong to ONE sample, so its guidance row and the weights are read once per
// workgroup (LDS in the forward, registers in the backward).  The sums run in a fixed order -- per workgroup over its rows, then
// over the workgroups' partial rows in the workspace (reduce.hip) -- no atomics: two runs give the same bits.
// tanh is vqf_tanh_fast (common.h): the value feeds a softmax logit, not a recursion.
#include "common.h"

namespace {

constexpr int GL_EMAX = 1024, GL_SMAX = 1024;
constexpr int GL_FWD_ROWS = 32;       // rows of a sample per forward workgroup (four waves, one row per wave and trip)
constexpr int GL_BWD_ROWS = 64;       // rows of a sample per backward workgroup (one partial row of dgp and of dw each)

// a sample's S rows in equal chunks of at most `cap` rows
inline int gl_chunks(int S, int cap) { return (S + cap - 1) / cap; }
inline int gl_rows(int S, int cap) { const int nc = gl_chunks(S, cap); return (S + nc - 1) / nc; }

// grid (chunks, N), 256 threads.  LDS: [gp[n] (G E) | w (G E)].  idx (N, or null: u = n; the grouped form): question n reads the
// Xh rows of sample u = idx[n], clamped to [0, U - 1] here, and writes its own logits rows.  A wave takes a row: lane q reads the 16-byte groups
// q, q + 64, ... of the row's G E contiguous floats (four loads in flight), the group's step is found by comparison.
// PACK (vqf_guided_logits_fwd_packed): Xh is (Rtot, ldx), the real rows of every owner one after the other, and roff holds the
// owners' row offsets; owner u has Sv rows from row0 by vqf_packed_span's rule (common.h), so whatever roff holds the rows read lie
// inside Xh.  logits stay (N*S, G): rows s >= Sv are written as exact zeros, no Xh row is read for them.
// (Without PACK the kernels of this file keep their own address expressions: their code is what it was before the flag.)
template <int G, bool PACK = false>
__global__ void __launch_bounds__(256) guided_logits_fwd_kernel(const float* __restrict__ Xh, int ldx, const float* __restrict__ gp,
                                                                const float* __restrict__ w, int S, int E, int rows,
                                                                float* __restrict__ logits, const int* __restrict__ idx, int U,
                                                                const int* __restrict__ roff, int Rtot) {
  extern __shared__ __attribute__((aligned(16))) float gl_lds[];
  const int GE = G * E, n = blockIdx.y;
  // (vqf_region_owner's rule, common.h, restated: through the helper the scalar prologue of all six instantiations came out in another
  // order -- same registers -- and no bench reaches G = 2)
  const int u = idx ? min(max(idx[n], 0), U - 1) : n;               // (uniform) the sample whose Xh rows this question reads
  long long row0 = 0;
  int Sv = S;                                                       // (uniform) the owner's real rows
  if (PACK) vqf_packed_span(roff, u, S, Rtot, row0, Sv);
  float* gs = gl_lds;
  float* ws = gl_lds + GE;
  for (int c = threadIdx.x * 4; c < GE; c += 1024) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(gs + c) = gp ? *reinterpret_cast<const f32x4*>(gp + (long long)n * GE + c) : zero;
    *reinterpret_cast<f32x4*>(ws + c) = *reinterpret_cast<const f32x4*>(w + c);
  }
  __syncthreads();
  const int s0 = blockIdx.x * rows, s1 = min(S, s0 + rows);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nq = GE >> 2;
  constexpr int UNR = 4;
  for (int s = s0 + wave; s < s1; s += 4) {
    const long long r = (long long)n * S + s;
    if (PACK && s >= Sv) {                                          // (wave-uniform) behind the count: zero logits, Xh unread
      if (lane < G) logits[(long long)G * r + lane] = 0.f;
      continue;
    }
    const float* x = PACK ? Xh + (row0 + s) * ldx : Xh + ((long long)u * S + s) * ldx;
    float a[G];
#pragma unroll
    for (int g = 0; g < G; ++g) a[g] = 0.f;
    for (int q0 = lane; q0 < nq; q0 += 64 * UNR) {
      f32x4 xv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int q = min(q0 + 64 * u, nq - 1);                    // past the end: re-read the last group (not used)
        xv[u] = vqf_ld_stream(reinterpret_cast<const f32x4*>(x + 4 * q));
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int c = 4 * (q0 + 64 * u);
        if (c >= GE) break;
        const f32x4 gv = *reinterpret_cast<const f32x4*>(gs + c);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + c);
        float p = vqf_tanh_fast(xv[u][0] + gv[0]) * wv[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) p += vqf_tanh_fast(xv[u][j] + gv[j]) * wv[j];
        const int lv = (G > 1 && c >= E) + (G > 2 && c >= 2 * E);
#pragma unroll
        for (int g = 0; g < G; ++g) a[g] += lv == g ? p : 0.f;
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float t = wave_sum(a[g]);
      if (lane == 0) logits[(long long)G * r + g] = t;
    }
  }
}

// grid (chunks, N), G E / 4 threads rounded up to whole waves: a thread owns four columns and walks the chunk's rows (four
// rows in flight), so gp[n], w and the two running sums stay in registers.  part_g / part_w: one row of G E floats per
// workgroup (row n * chunks + chunk); with one chunk per sample part_g is dgp itself.
// PACK (vqf_guided_logits_bwd_packed, plain form): Xh and dXh are (Rtot, .) packed, sample n's Sv rows from row0 (vqf_packed_span);
// dl stays (N*S, G).  The chunks are those of S: a chunk stops at Sv (rows behind it are neither read nor written, dl included),
// a chunk wholly behind the count writes zero partial rows -- the partial-row layout, and with it the order of the dgp and dw
// sums, is that of the padded kernel.
template <int G, bool PACK = false>
__global__ void __launch_bounds__(768) guided_logits_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ Xh, int ldx,
                                                                const float* __restrict__ gp, const float* __restrict__ w, int S,
                                                                int E, int rows, float* __restrict__ dXh, int ldd,
                                                                float* __restrict__ part_g, float* __restrict__ part_w,
                                                                const int* __restrict__ roff, int Rtot) {
  const int GE = G * E, n = blockIdx.y;
  const int c = threadIdx.x * 4;
  if (c >= GE) return;
  long long row0 = 0;
  int Sv = S;
  if (PACK) vqf_packed_span(roff, n, S, Rtot, row0, Sv);
  const int s0 = blockIdx.x * rows, s1 = min(Sv, s0 + rows);
  const int lv = (G > 1 && c >= E) + (G > 2 && c >= 2 * E);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 gv = gp ? *reinterpret_cast<const f32x4*>(gp + (long long)n * GE + c) : zero;
  const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
  f32x4 sg = zero, sw = zero;
  const long long r0 = (long long)n * S;
  const long long x0 = PACK ? row0 : r0;                           // the first of the sample's rows in Xh / dXh
  constexpr int RB = 4;
  for (int sb = s0; sb < s1; sb += RB) {
    f32x4 x[RB];
    float d[RB];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const int sq = min(sb + q, s1 - 1);                          // the tail trip re-reads the last row (not used)
      x[q] = vqf_ld_stream(reinterpret_cast<const f32x4*>(Xh + (x0 + sq) * ldx + c));
      d[q] = dl[(long long)G * (r0 + sq) + lv];
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      if (sb + q >= s1) break;
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float h = vqf_tanh_fast(x[q][j] + gv[j]);
        o[j] = (d[q] * wv[j]) * (1.0f - h * h);
        sg[j] += o[j];
        sw[j] += d[q] * h;
      }
      *reinterpret_cast<f32x4*>(dXh + (x0 + sb + q) * ldd + c) = o;
    }
  }
  const long long prow = ((long long)n * gridDim.x + blockIdx.x) * GE + c;
  *reinterpret_cast<f32x4*>(part_g + prow) = sg;
  *reinterpret_cast<f32x4*>(part_w + prow) = sw;
}

// The grouped backward: Xh (U*S, .) is shared by the questions of an image.  grid (chunks, U), the thread layout of the kernel
// above.  A workgroup owns `rows` rows of image u and walks that image's questions order[grp_off[u]] .. order[grp_off[u + 1] - 1]
// in that order, GL_GRP_Q at a time (their guidance rows and dgp sums in registers): the first pass over the rows writes
// dXh[u] = the pass's sum, each later pass adds to what the same thread wrote -- a fixed order, no atomics.  part_g: row
// n * chunks + chunk (each question is in one group: written once); part_w: row u * chunks + chunk.  An empty group writes zero
// dXh rows and a zero part_w row.  grp_off and order are clamped to [0, N] / [0, N - 1] here: nothing they hold reads out of range.
// PACK (vqf_guided_logits_bwd_packed, grouped form): Xh and dXh are (Rtot, .) packed, image u's Sv rows from row0; dl stays
// (N*S, G).  A chunk stops at Sv as in the plain kernel above; an empty group writes zeros on the image's Sv rows.
constexpr int GL_GRP_Q = 4;

template <int G, bool PACK = false>
__global__ void __launch_bounds__(768) guided_logits_bwd_grouped_kernel(const float* __restrict__ dl, const float* __restrict__ Xh,
                                                                        int ldx, const float* __restrict__ gp,
                                                                        const float* __restrict__ w, const int* __restrict__ order,
                                                                        const int* __restrict__ grp_off, int N, int S, int E, int rows,
                                                                        float* __restrict__ dXh, int ldd, float* __restrict__ part_g,
                                                                        float* __restrict__ part_w, const int* __restrict__ roff,
                                                                        int Rtot) {
  const int GE = G * E, u = blockIdx.y;
  const int c = threadIdx.x * 4;
  if (c >= GE) return;
  long long row0 = 0;
  int Sv = S;
  if (PACK) vqf_packed_span(roff, u, S, Rtot, row0, Sv);
  const int s0 = blockIdx.x * rows, s1 = min(Sv, s0 + rows);
  const int lv = (G > 1 && c >= E) + (G > 2 && c >= 2 * E);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
  int jb, je;
  vqf_group_range(grp_off, u, N, jb, je);
  const long long r0 = PACK ? row0 : (long long)u * S;              // the first of the image's rows in Xh / dXh
  f32x4 sw = zero;
  if (jb == je)
    for (int s = s0; s < s1; ++s) *reinterpret_cast<f32x4*>(dXh + (r0 + s) * ldd + c) = zero;
  for (int j0 = jb; j0 < je; j0 += GL_GRP_Q) {
    const int nq = min(GL_GRP_Q, je - j0);
    int nn[GL_GRP_Q];
    f32x4 gv[GL_GRP_Q], sg[GL_GRP_Q];
#pragma unroll
    for (int q = 0; q < GL_GRP_Q; ++q) {                            // past the group's end: the last question again (not used)
      nn[q] = vqf_group_member(order, j0 + q, je, N);
      gv[q] = *reinterpret_cast<const f32x4*>(gp + (long long)nn[q] * GE + c);
      sg[q] = zero;
    }
    for (int s = s0; s < s1; ++s) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(Xh + (r0 + s) * ldx + c);
      f32x4 o = j0 == jb ? zero : *reinterpret_cast<const f32x4*>(dXh + (r0 + s) * ldd + c);
      float d[GL_GRP_Q];
#pragma unroll
      for (int q = 0; q < GL_GRP_Q; ++q) d[q] = dl[(long long)G * ((long long)nn[q] * S + s) + lv];
#pragma unroll
      for (int q = 0; q < GL_GRP_Q; ++q) {
        if (q >= nq) break;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float h = vqf_tanh_fast(x[j] + gv[q][j]);
          const float t = (d[q] * wv[j]) * (1.0f - h * h);
          o[j] += t;
          sg[q][j] += t;
          sw[j] += d[q] * h;
        }
      }
      *reinterpret_cast<f32x4*>(dXh + (r0 + s) * ldd + c) = o;
    }
#pragma unroll
    for (int q = 0; q < GL_GRP_Q; ++q)
      if (q < nq) *reinterpret_cast<f32x4*>(part_g + ((long long)nn[q] * gridDim.x + blockIdx.x) * GE + c) = sg[q];
  }
  *reinterpret_cast<f32x4*>(part_w + ((long long)u * gridDim.x + blockIdx.x) * GE + c) = sw;
}

// ---- the launchers of every form, behind the refusals of its entry point.  rg (VqfRegions, common.h; host side only) says where
// the Xh rows are: U owners (the plain forms fill U = N), idx / order + grp_off when questions share them, roff / Rtot when packed.
int guided_fwd_launch(const float* Xh, int ldx, const float* gp, const float* w, int N, int S, int E, int G, float* logits,
                      void* stream, const VqfRegions& rg) {
  if (!aligned16(Xh) || !aligned16(gp) || !aligned16(w)) return VQF_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int rows = gl_rows(S, GL_FWD_ROWS);
  const dim3 grid(gl_chunks(S, rows), N);
  const size_t lds = (size_t)2 * G * E * sizeof(float);
  auto go = [&](auto g, auto pack) {
    VQF_LAUNCH(KID_GUIDED_FWD, (guided_logits_fwd_kernel<decltype(g)::value, decltype(pack)::value>), grid, dim3(256), lds, s, Xh,
               ldx, gp, w, S, E, rows, logits, rg.idx, rg.U, rg.roff, rg.Rtot);
  };
  vqf_dispatch_G(G, [&](auto g) { if (rg.packed()) go(g, std::true_type()); else go(g, std::false_type()); });
  return vqf_last_error();
}

// ws: part_w (U * chunks rows of G E), then part_g (N * chunks rows; dgp itself with one chunk), then the reducer's
// VQF_REDUCE_SPLITS rows.  The plain form is U = N: part_w, part_g with nb = N * chunks rows each, the layout it always had.
// The chunks are those of S in the packed forms too: the padded kernels' partial rows.
int guided_bwd_launch(const float* dlogits, const float* Xh, int ldx, const float* gp, const float* w, int N, int S, int E, int G,
                      float* dXh, int lddx, float* dgp, float* dw, void* ws, size_t ws_bytes, void* stream, const VqfRegions& rg) {
  if (!aligned16(Xh) || !aligned16(gp) || !aligned16(w) || !aligned16(dXh) || !aligned16(dgp) || !aligned16(ws)) return VQF_E_ALIGN;
  if (!ws || ws_bytes < vqf_guided_logits_bwd_grouped_ws_bytes(N, rg.U, S, E, G)) return VQF_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int GE = G * E, U = rg.U;
  const int rows = gl_rows(S, GL_BWD_ROWS), chunks = gl_chunks(S, rows);
  float* part_w = (float*)ws;
  float* part_g = chunks == 1 ? dgp : part_w + (size_t)U * chunks * GE;
  float* scratch = part_w + ((size_t)U + N) * chunks * GE;
  const dim3 grid(chunks, U), block(((GE / 4 + 63) / 64) * 64);
  auto own = [&](auto g, auto pack) {
    VQF_LAUNCH(KID_GUIDED_BWD, (guided_logits_bwd_kernel<decltype(g)::value, decltype(pack)::value>), grid, block, 0, s, dlogits, Xh,
               ldx, gp, w, S, E, rows, dXh, lddx, part_g, part_w, rg.roff, rg.Rtot);
  };
  auto shared = [&](auto g, auto pack) {
    VQF_LAUNCH(KID_GUIDED_BWD, (guided_logits_bwd_grouped_kernel<decltype(g)::value, decltype(pack)::value>), grid, block, 0, s,
               dlogits, Xh, ldx, gp, w, rg.order, rg.grp_off, N, S, E, rows, dXh, lddx, part_g, part_w, rg.roff, rg.Rtot);
  };
  vqf_dispatch_G(G, [&](auto g) {
    if (rg.grouped()) { if (rg.packed()) shared(g, std::true_type()); else shared(g, std::false_type()); }
    else if (rg.packed()) own(g, std::true_type());
    else own(g, std::false_type());
  });
  int rc = vqf_last_error();
  if (rc) return rc;
  if (chunks > 1) {
    rc = vqf_group_reduce_f32(part_g, N, chunks, GE, dgp, stream);           // dgp[n] = its chunks' rows, in chunk order
    if (rc) return rc;
  }
  return vqf_colreduce_2stage(part_w, U * chunks, GE, dw, scratch, s);
}

}  // namespace

extern "C" {

int vqf_guided_logits_supported(int N, int S, int E, int G) {
  return N >= 1 && N <= 65535 && S >= 1 && S <= GL_SMAX && E >= 32 && E <= GL_EMAX && (E % 32) == 0 && G >= 1 && G <= 3 &&
         (long long)N * S < (1LL << 31) / 4;
}

int vqf_guided_logits_fwd(const float* Xh, int ldx, const float* gp, const float* w, int N, int S, int E, int G, float* logits,
                          void* stream) {
  if (!Xh || !w || !logits || N <= 0 || S <= 0 || E <= 0 || G <= 0 || ldx < G * E || (ldx % 4)) return VQF_E_BADARG;
  if (!vqf_guided_logits_supported(N, S, E, G)) return VQF_E_UNSUPPORTED;
  return guided_fwd_launch(Xh, ldx, gp, w, N, S, E, G, logits, stream, {.U = N});
}

int vqf_guided_logits_grouped_supported(int N, int U, int S, int E, int G) {
  return vqf_guided_logits_supported(N, S, E, G) && U >= 1 && U <= 65535 && (long long)U * S < (1LL << 31) / 4;
}

int vqf_guided_logits_fwd_grouped(const float* Xh, int ldx, const float* gp, const float* w, const int* idx, int N, int U, int S,
                                  int E, int G, float* logits, void* stream) {
  if (!Xh || !gp || !w || !VqfRegions::ok(idx) || !logits || N <= 0 || U <= 0 || S <= 0 || E <= 0 || G <= 0 || ldx < G * E ||
      (ldx % 4))
    return VQF_E_BADARG;
  if (!vqf_guided_logits_grouped_supported(N, U, S, E, G)) return VQF_E_UNSUPPORTED;
  return guided_fwd_launch(Xh, ldx, gp, w, N, S, E, G, logits, stream, {.idx = idx, .U = U});
}

size_t vqf_guided_logits_bwd_ws_bytes(int N, int S, int E, int G) {
  if (N <= 0 || S <= 0 || E <= 0 || G <= 0) return 0;
  const size_t nb = (size_t)N * gl_chunks(S, gl_rows(S, GL_BWD_ROWS));
  return (2 * nb + VQF_REDUCE_SPLITS) * (size_t)G * E * sizeof(float);       // dgp partial rows, dw partial rows, reduction scratch
}

int vqf_guided_logits_bwd(const float* dlogits, const float* Xh, int ldx, const float* gp, const float* w, int N, int S, int E,
                          int G, float* dXh, int lddx, float* dgp, float* dw, void* ws, size_t ws_bytes, void* stream) {
  if (!dlogits || !Xh || !w || !dXh || !dgp || !dw || N <= 0 || S <= 0 || E <= 0 || G <= 0 || ldx < G * E || lddx < G * E ||
      (ldx % 4) || (lddx % 4))
    return VQF_E_BADARG;
  if (!vqf_guided_logits_supported(N, S, E, G)) return VQF_E_UNSUPPORTED;
  return guided_bwd_launch(dlogits, Xh, ldx, gp, w, N, S, E, G, dXh, lddx, dgp, dw, ws, ws_bytes, stream, {.U = N});
}

size_t vqf_guided_logits_bwd_grouped_ws_bytes(int N, int U, int S, int E, int G) {
  if (N <= 0 || U <= 0 || S <= 0 || E <= 0 || G <= 0) return 0;
  const size_t chunks = gl_chunks(S, gl_rows(S, GL_BWD_ROWS));
  return (((size_t)N + U) * chunks + VQF_REDUCE_SPLITS) * (size_t)G * E * sizeof(float);   // dgp rows, dw rows, reduction scratch
}

int vqf_guided_logits_bwd_grouped(const float* dlogits, const float* Xh, int ldx, const float* gp, const float* w, const int* order,
                                  const int* grp_off, int N, int U, int S, int E, int G, float* dXh, int lddx, float* dgp, float* dw,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (!dlogits || !Xh || !gp || !w || !VqfRegions::ok(order) || !VqfRegions::ok(grp_off) || !dXh || !dgp || !dw || N <= 0 ||
      U <= 0 || S <= 0 || E <= 0 || G <= 0 || ldx < G * E || lddx < G * E || (ldx % 4) || (lddx % 4))
    return VQF_E_BADARG;
  if (!vqf_guided_logits_grouped_supported(N, U, S, E, G)) return VQF_E_UNSUPPORTED;
  return guided_bwd_launch(dlogits, Xh, ldx, gp, w, N, S, E, G, dXh, lddx, dgp, dw, ws, ws_bytes, stream,
                           {.order = order, .grp_off = grp_off, .U = U});
}

// ---- the packed forms: Xh / dXh (R, .) hold the real rows only, roff (owners + 1) int32 row offsets --------------------------
int vqf_guided_logits_packed_supported(int N, int U, int R, int S, int E, int G) {
  return vqf_guided_logits_grouped_supported(N, U, S, E, G) && R >= 1 && R < (1 << 29);
}

// what both packed entry points refuse after their operands; own = idx / order decides the form (NULL: plain, U must equal N)
static int guided_packed_refusal(const int* own, const VqfRegions& rg, int N, int S, int E, int G) {
  if (!rg.packed_ok(own, N) || N <= 0 || S <= 0 || E <= 0 || G <= 0) return VQF_E_BADARG;
  return vqf_guided_logits_packed_supported(N, rg.U, rg.Rtot, S, E, G) ? VQF_OK : VQF_E_UNSUPPORTED;
}

int vqf_guided_logits_fwd_packed(const float* Xh, int ldx, const float* gp, const float* w, const int* idx, const int* roff, int N,
                                 int U, int R, int S, int E, int G, float* logits, void* stream) {
  if (!Xh || !w || !logits || ldx < G * E || (ldx % 4)) return VQF_E_BADARG;
  const VqfRegions rg = {.idx = idx, .U = U, .roff = roff, .Rtot = R};
  const int rc = guided_packed_refusal(idx, rg, N, S, E, G);
  return rc ? rc : guided_fwd_launch(Xh, ldx, gp, w, N, S, E, G, logits, stream, rg);
}

size_t vqf_guided_logits_bwd_packed_ws_bytes(int N, int U, int S, int E, int G) {
  return vqf_guided_logits_bwd_grouped_ws_bytes(N, U, S, E, G);              // U = N in the plain form: the layout of the plain kernel
}

int vqf_guided_logits_bwd_packed(const float* dlogits, const float* Xh, int ldx, const float* gp, const float* w, const int* order,
                                 const int* grp_off, const int* roff, int N, int U, int R, int S, int E, int G, float* dXh, int lddx,
                                 float* dgp, float* dw, void* ws, size_t ws_bytes, void* stream) {
  if (!dlogits || !Xh || !w || !dXh || !dgp || !dw || ldx < G * E || lddx < G * E || (ldx % 4) || (lddx % 4) ||
      (order != nullptr) != (grp_off != nullptr) || (order && !gp) || !VqfRegions::aligned(grp_off))
    return VQF_E_BADARG;
  const VqfRegions rg = {.order = order, .grp_off = grp_off, .U = U, .roff = roff, .Rtot = R};
  const int rc = guided_packed_refusal(order, rg, N, S, E, G);
  return rc ? rc : guided_bwd_launch(dlogits, Xh, ldx, gp, w, N, S, E, G, dXh, lddx, dgp, dw, ws, ws_bytes, stream, rg);
}

}  // extern "C"

