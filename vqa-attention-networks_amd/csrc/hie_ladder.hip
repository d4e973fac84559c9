// The word / phrase / sentence co-attention ladder (HieCoAttenLadder, host/hie_ladder.py; Lu et al. 2016): the two stages
// the single-level HieCoAtten kernels (hie.hip) do not cover.
//
// Phrase level.  The unigram, bigram and trigram convolutions over the word features Qw (N, T, E) (right zero padding: the
// window of position t is t .. t + k - 1) are ONE GEMM on the fp32 kernels, Z = Qw Wcat^T with the six taps stacked,
//   Wcat (6E, E) = [W1[:,:,0] | W2[:,:,0] W2[:,:,1] | W3[:,:,0] W3[:,:,1] W3[:,:,2]]      (tap (k, j) at column block k(k-1)/2 + j)
// and the rest is one streaming pass over Z here:
//   u_k[t] = b_k + sum_{j < k, t + j < T} Z[n, t + j, tap(k, j)]
//   Qp[t]  = tanh(max_k u_k[t])        (tanh is monotonic: the maximum is taken on u, one tanh per element)
//   idx[t] = the winning k - 1         (the first maximum on a tie: k = 1 before 2 before 3)
// The backward gives du = dQp (1 - Qp^2) to the winning k and writes dZ (N*T, 6E) as a GATHER: row r of tap (k, j) reads the
// output r - j of the same sample (no atomics, every element written once).  The column sums of dZ's j = 0 taps are the three
// bias gradients; dQw and dWcat are GEMMs on the existing kernels.  T <= 32 (the windows of a sample stay in one workgroup's
// reach), E % 4 == 0.
//
// Multi-level affinity.  C_g[n, t, l] = sum_e X_g[n, t, e] Y_g[n, l, e] for G <= 3 levels in ONE pass over the y rows: the
// three levels of the ladder attend over the same image tensor V, so the forward (C_g = tanh(Cq_g V^T)) reads V once instead
// of three times.  X_g are the rows of x at column offset g * ldx_level; Y_g those of y at g * ldy_level (0: one shared y,
// loaded once per k slab and fed to all G accumulators).  An optional second pair (x2, y2) is accumulated behind the first
// (the backward's dC_g = dti_g Vh_g^T + Qh_g dtq_g^T).  Epilogue 0: the products; 1: tanh; 2: the tanh backward given the
// forward's output yprev (v (1 - yprev^2)).  No dropout (the ladder has none on C).  The k order of a level is that of
// vqf_hie_affinity (hie.hip): G = 1 gives the same bits.  out and yprev: (G, N, T, L), contiguous per level.
#include "common.h"

namespace {

constexpr int PH_TMAX = 32;

// one thread per (row, 4 columns); rows r = n * T + t
__global__ void phrase_ngram_fwd_kernel(const float* __restrict__ Z, int ldz, const float* __restrict__ bias, int NT, int T,
                                        int E, float* __restrict__ Qp, int ldq, uint8_t* __restrict__ idx) {
  const int CT = E >> 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)NT * CT) return;
  const int r = (int)(i / CT), c = 4 * (int)(i - (long long)r * CT);
  const int t = r % T;
  const float* z0 = Z + (long long)r * ldz + c;
  const bool h1 = t + 1 < T, h2 = t + 2 < T;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 u1t0 = *reinterpret_cast<const f32x4*>(z0);
  const f32x4 u2t0 = *reinterpret_cast<const f32x4*>(z0 + E);
  const f32x4 u2t1 = h1 ? *reinterpret_cast<const f32x4*>(z0 + ldz + 2 * E) : zero;
  const f32x4 u3t0 = *reinterpret_cast<const f32x4*>(z0 + 3 * E);
  const f32x4 u3t1 = h1 ? *reinterpret_cast<const f32x4*>(z0 + ldz + 4 * E) : zero;
  const f32x4 u3t2 = h2 ? *reinterpret_cast<const f32x4*>(z0 + 2 * (long long)ldz + 5 * E) : zero;
  const f32x4 b1 = *reinterpret_cast<const f32x4*>(bias + c);
  const f32x4 b2 = *reinterpret_cast<const f32x4*>(bias + E + c);
  const f32x4 b3 = *reinterpret_cast<const f32x4*>(bias + 2 * E + c);
  f32x4 q;
  uint32_t packed = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float u1 = b1[j] + u1t0[j];
    const float u2 = (b2[j] + u2t0[j]) + u2t1[j];
    const float u3 = ((b3[j] + u3t0[j]) + u3t1[j]) + u3t2[j];
    float m = u1;
    uint32_t k = 0;
    if (u2 > m) { m = u2; k = 1; }
    if (u3 > m) { m = u3; k = 2; }
    q[j] = tanhf(m);
    packed |= k << (8 * j);
  }
  *reinterpret_cast<f32x4*>(Qp + (long long)r * ldq + c) = q;
  *reinterpret_cast<uint32_t*>(idx + (long long)r * E + c) = packed;
}

// dZ[r, tap(k, j)] = (t - j >= 0 && idx[r - j] == k - 1) ? du[r - j] : 0,  du = dQp (1 - Qp^2)
__global__ void phrase_ngram_bwd_kernel(const float* __restrict__ dQp, int ldd, const float* __restrict__ Qp, int ldq,
                                        const uint8_t* __restrict__ idx, int NT, int T, int E, float* __restrict__ dZ, int ldz) {
  const int CT = E >> 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)NT * CT) return;
  const int r = (int)(i / CT), c = 4 * (int)(i - (long long)r * CT);
  const int t = r % T;
  f32x4 du[3];
  uint32_t win[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {                   // the outputs r, r - 1, r - 2 of the same sample
    du[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    win[j] = 0xFFFFFFFFu;
    if (t - j >= 0) {
      const long long rr = r - j;
      const f32x4 d = *reinterpret_cast<const f32x4*>(dQp + rr * ldd + c);
      const f32x4 q = *reinterpret_cast<const f32x4*>(Qp + rr * ldq + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) du[j][e] = d[e] * (1.0f - q[e] * q[e]);
      win[j] = *reinterpret_cast<const uint32_t*>(idx + rr * E + c);
    }
  }
  float* zr = dZ + (long long)r * ldz + c;
#pragma unroll
  for (int k = 1; k <= 3; ++k)
#pragma unroll
    for (int j = 0; j < k; ++j) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = ((win[j] >> (8 * e)) & 0xFFu) == (uint32_t)(k - 1) ? du[j][e] : 0.f;
      *reinterpret_cast<f32x4*>(zr + (k * (k - 1) / 2 + j) * E) = o;
    }
}

struct AffLvArgs {
  const float* x1; int ldx1, lvx1; const float* y1; int ldy1, lvy1;
  const float* x2; int ldx2, lvx2; const float* y2; int ldy2, lvy2;
  const float* yprev; float* out;
  int G, N, L, E, T;
};

// hie_affinity_kernel (hie.hip) with G levels: LDS holds the G x npair (16, E) X images (rows T..15 zero); a wave owns 16 y rows
template <int EPI>
__global__ void __launch_bounds__(1024) hie_affinity_levels_kernel(const AffLvArgs g) {
  extern __shared__ float smem[];
  const int E = g.E, T = g.T, L = g.L, ES = E + 4, G = g.G;
  const int n = blockIdx.y, tid = threadIdx.x, W = blockDim.x >> 6, wave = tid >> 6, lane = tid & 63;
  const int npair = g.x2 ? 2 : 1, CT = E >> 2;
  for (int p = 0; p < npair; ++p)
    for (int lv = 0; lv < G; ++lv) {
      const float* x = (p ? g.x2 + lv * g.lvx2 : g.x1 + lv * g.lvx1);
      const int ldx = p ? g.ldx2 : g.ldx1;
      float* Xs = smem + (p * G + lv) * 16 * ES;
      for (int i = tid; i < 16 * CT; i += blockDim.x) {
        const int t = i / CT, c = i - t * CT;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t < T) v = *reinterpret_cast<const f32x4*>(x + (long long)(n * T + t) * ldx + 4 * c);
        *reinterpret_cast<f32x4*>(Xs + t * ES + 4 * c) = v;
      }
    }
  __syncthreads();
  const int NG = (L + 15) >> 4;
  const int r = lane & 15, kq = lane >> 4;
  for (int grp = blockIdx.x * W + wave; grp < NG; grp += gridDim.x * W) {
    const int l = grp * 16 + r;
    const long long row = (long long)n * L + (l < L ? l : L - 1);      // rows past L: a valid row, result not stored
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int p = 0; p < npair; ++p) {
      const int lvy = p ? g.lvy2 : g.lvy1;
      const float* y0 = (p ? g.y2 : g.y1) + row * (p ? g.ldy2 : g.ldy1) + 8 * kq;
      for (int k0 = 0; k0 < E; k0 += 256) {
        f32x4 b[16];
#pragma unroll
        for (int lv = 0; lv < 3; ++lv) {
          if (lv >= G) break;                                           // (uniform)
          if (lv == 0 || lvy != 0) {                                    // a shared y is loaded once per k slab
            const float* y = y0 + lv * lvy;
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if (k0 + 32 * u < E) {
                b[2 * u] = vqf_ld_stream(reinterpret_cast<const f32x4*>(y + k0 + 32 * u));
                b[2 * u + 1] = vqf_ld_stream(reinterpret_cast<const f32x4*>(y + k0 + 32 * u + 4));
              }
          }
          const float* xs = smem + (p * G + lv) * 16 * ES + r * ES + 8 * kq;
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (k0 + 32 * u < E) {
              const f32x4 a0 = *reinterpret_cast<const f32x4*>(xs + k0 + 32 * u);
              const f32x4 a1 = *reinterpret_cast<const f32x4*>(xs + k0 + 32 * u + 4);
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[lv] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], b[2 * u][j], acc[lv], 0, 0, 0);
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[lv] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], b[2 * u + 1][j], acc[lv], 0, 0, 0);
            }
        }
      }
    }
    if (l < L) {
#pragma unroll
      for (int lv = 0; lv < 3; ++lv) {
        if (lv >= G) break;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int t = 4 * kq + j;                                    // D: rows 4 (lane / 16) + j, column lane % 16
          if (t < T) {
            const long long idx = (((long long)lv * g.N + n) * T + t) * L + l;
            float v = acc[lv][j];
            if (EPI == 1) {
              v = vqf_tanh_fast(v);
            } else if (EPI == 2) {
              const float th = g.yprev[idx];
              v = v * (1.0f - th * th);
            }
            g.out[idx] = v;
          }
        }
      }
    }
  }
}

VqfDynLdsFlags g_afflv_lds[3];

bool rows_ok(const float* p, int ld, int E) { return p && aligned16(p) && ld >= E && (ld % 4) == 0; }

}  // namespace

extern "C" {

int vqf_phrase_ngram_supported(int T, int E) {
  return T >= 1 && T <= PH_TMAX && E >= 4 && (E % 4) == 0;
}

int vqf_phrase_ngram_fwd(const float* Z, int ldz, const float* bias, int N, int T, int E, float* Qp, int ldq, uint8_t* idx,
                         void* stream) {
  if (!Z || !bias || !Qp || !idx || N <= 0 || ldz < 6 * E || ldq < E || (ldz % 4) || (ldq % 4)) return VQF_E_BADARG;
  if (!vqf_phrase_ngram_supported(T, E) || (long long)N * T * (E / 4) >= (1LL << 31)) return VQF_E_UNSUPPORTED;
  if (!aligned16(Z) || !aligned16(bias) || !aligned16(Qp) || (((uintptr_t)idx) & 3)) return VQF_E_ALIGN;
  const long long n4 = (long long)N * T * (E / 4);
  VQF_LAUNCH(KID_PHRASE_FWD, phrase_ngram_fwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Z, ldz,
             bias, N * T, T, E, Qp, ldq, idx);
  return vqf_last_error();
}

int vqf_phrase_ngram_bwd(const float* dQp, int ldd, const float* Qp, int ldq, const uint8_t* idx, int N, int T, int E, float* dZ,
                         int ldz, void* stream) {
  if (!dQp || !Qp || !idx || !dZ || N <= 0 || ldz < 6 * E || ldq < E || ldd < E || (ldz % 4) || (ldq % 4) || (ldd % 4))
    return VQF_E_BADARG;
  if (!vqf_phrase_ngram_supported(T, E) || (long long)N * T * (E / 4) >= (1LL << 31)) return VQF_E_UNSUPPORTED;
  if (!aligned16(dQp) || !aligned16(Qp) || !aligned16(dZ) || (((uintptr_t)idx) & 3)) return VQF_E_ALIGN;
  const long long n4 = (long long)N * T * (E / 4);
  VQF_LAUNCH(KID_PHRASE_BWD, phrase_ngram_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dQp,
             ldd, Qp, ldq, idx, N * T, T, E, dZ, ldz);
  return vqf_last_error();
}

int vqf_hie_affinity_levels_supported(int N, int L, int E, int T, int G, int pairs) {
  if (N <= 0 || N > 65535 || L <= 0 || T <= 0 || T > 16 || E <= 0 || (E % 32) || G < 1 || G > 3 || pairs < 1 || pairs > 2)
    return 0;
  return (size_t)G * pairs * 16 * (E + 4) * sizeof(float) <= 160 * 1024;
}

int vqf_hie_affinity_levels(const float* x1, int ldx1, int ldx_level1, const float* y1, int ldy1, int ldy_level1,
                            const float* x2, int ldx2, int ldx_level2, const float* y2, int ldy2, int ldy_level2,
                            int G, int epi, const float* yprev, int N, int L, int E, int T, float* out, void* stream) {
  const int pairs = x2 ? 2 : 1;
  if (!out || !rows_ok(x1, ldx1, E) || !rows_ok(y1, ldy1, E) || (!x2) != (!y2) || (x2 && (!rows_ok(x2, ldx2, E) || !rows_ok(y2, ldy2, E))) ||
      epi < 0 || epi > 2 || (epi == 2 && !yprev) || ldx_level1 < 0 || ldy_level1 < 0 || (ldx_level1 % 4) || (ldy_level1 % 4) ||
      (x2 && (ldx_level2 < 0 || ldy_level2 < 0 || (ldx_level2 % 4) || (ldy_level2 % 4))))
    return VQF_E_BADARG;
  if (!vqf_hie_affinity_levels_supported(N, L, E, T, G, pairs)) return VQF_E_UNSUPPORTED;
  // every level's columns stay inside the row (a level offset plus E within the row pitch)
  if ((G - 1) * ldx_level1 + E > ldx1 || (G - 1) * ldy_level1 + E > ldy1 ||
      (x2 && ((G - 1) * ldx_level2 + E > ldx2 || (G - 1) * ldy_level2 + E > ldy2)))
    return VQF_E_BADARG;
  AffLvArgs g = {};
  g.x1 = x1; g.ldx1 = ldx1; g.lvx1 = ldx_level1; g.y1 = y1; g.ldy1 = ldy1; g.lvy1 = ldy_level1;
  g.x2 = x2; g.ldx2 = ldx2; g.lvx2 = ldx_level2; g.y2 = y2; g.ldy2 = ldy2; g.lvy2 = ldy_level2;
  g.yprev = yprev; g.out = out; g.G = G; g.N = N; g.L = L; g.E = E; g.T = T;
  const int cus = vqf_cu_count() > 0 ? vqf_cu_count() : 256;
  const int NG = (L + 15) / 16;
  int S = (cus + N - 1) / N;                       // whole samples per workgroup once N >= the CU count
  if (S > NG) S = NG;
  int W = (NG + S - 1) / S;
  if (W > 16) W = 16;
  const int lds = G * pairs * 16 * (E + 4) * (int)sizeof(float);
  const void* fn = epi == 0 ? (const void*)hie_affinity_levels_kernel<0>
                 : epi == 1 ? (const void*)hie_affinity_levels_kernel<1> : (const void*)hie_affinity_levels_kernel<2>;
  if (lds > 64 * 1024) {
    const int rc = vqf_set_dyn_lds(fn, lds, g_afflv_lds[epi]);
    if (rc != VQF_OK) return rc;
  }
  const dim3 grid(S, N), block(64 * W);
  hipStream_t s = (hipStream_t)stream;
  switch (epi) {
    case 0:  VQF_LAUNCH(KID_HIE_AFF_LEVELS, hie_affinity_levels_kernel<0>, grid, block, lds, s, g); break;
    case 1:  VQF_LAUNCH(KID_HIE_AFF_LEVELS, hie_affinity_levels_kernel<1>, grid, block, lds, s, g); break;
    default: VQF_LAUNCH(KID_HIE_AFF_LEVELS, hie_affinity_levels_kernel<2>, grid, block, lds, s, g); break;
  }
  return vqf_last_error();
}

}  // extern "C"
