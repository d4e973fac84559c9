// The word / phrase / sentence co-attention ladder (HieCoAttenLadder, host/hie_ladder.py; Lu et al. 2016): the phrase level.
// (Its multi-level affinity is hie_affinity_kernel of hie.hip, instantiated for up to three levels.)
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
// Question lengths (the *_len entry points; lens (N) int32, len[n] real words, the rest of the T positions padding): the window
// of position t stops at len[n] instead of T, a padded output row is zero with idx = 3 (no winner), and the backward writes
// zeros to the padded rows of dZ -- nothing is scattered to or from padding.  lens = null is the unmasked form, same bits.
//
// vqf_tanh_bwd_rows_len: dx = dy (1 - y^2) on the real rows of a contiguous (N, T, L) tensor, zero on the padded ones (the
// ladder's dC on the batched-GEMM route, T > 16; the streaming route masks in the affinity epilogue of hie.hip).
#include "common.h"

namespace {

constexpr int PH_TMAX = 32;

// one thread per (row, 4 columns); rows r = n * T + t
__global__ void phrase_ngram_fwd_kernel(const float* __restrict__ Z, int ldz, const float* __restrict__ bias, int NT, int T,
                                        int E, float* __restrict__ Qp, int ldq, uint8_t* __restrict__ idx,
                                        const int* __restrict__ lens) {
  const int CT = E >> 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)NT * CT) return;
  const int r = (int)(i / CT), c = 4 * (int)(i - (long long)r * CT);
  const int t = r % T, len = vqf_region_count(lens, r / T, T);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (t >= len) {                                   // a padded row: zero, no winner
    *reinterpret_cast<f32x4*>(Qp + (long long)r * ldq + c) = zero;
    *reinterpret_cast<uint32_t*>(idx + (long long)r * E + c) = 0x03030303u;
    return;
  }
  const float* z0 = Z + (long long)r * ldz + c;
  const bool h1 = t + 1 < len, h2 = t + 2 < len;
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
                                        const uint8_t* __restrict__ idx, int NT, int T, int E, float* __restrict__ dZ, int ldz,
                                        const int* __restrict__ lens) {
  const int CT = E >> 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)NT * CT) return;
  const int r = (int)(i / CT), c = 4 * (int)(i - (long long)r * CT);
  const int t = r % T;
  const bool real = t < vqf_region_count(lens, r / T, T);  // a padded row of Z entered no window: its dZ is zero
  f32x4 du[3];
  uint32_t win[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {                   // the outputs r, r - 1, r - 2 of the same sample
    du[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    win[j] = 0xFFFFFFFFu;
    if (real && t - j >= 0) {
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

// dx[n, t, l] = t < len[n] ? dy (1 - y^2) : 0 over a contiguous (N, T, L) tensor, four elements per thread (a group of four may
// straddle two rows when L % 4 != 0: the row is found per element)
__global__ void tanh_bwd_rows_len_kernel(const float* __restrict__ dy, const float* __restrict__ y, const int* __restrict__ lens,
                                         long long n4, int T, int L, float* __restrict__ dx) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 d = *reinterpret_cast<const f32x4*>(dy + 4 * i);
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + 4 * i);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long row = (4 * i + j) / L;
      const int n = (int)(row / T), t = (int)(row - (long long)n * T);
      o[j] = t < vqf_region_count(lens, n, T) ? d[j] * (1.0f - v[j] * v[j]) : 0.f;
    }
    *reinterpret_cast<f32x4*>(dx + 4 * i) = o;
  }
}

int phrase_fwd_launch(const float* Z, int ldz, const float* bias, const int* lens, int N, int T, int E, float* Qp, int ldq,
                      uint8_t* idx, void* stream) {
  if (!Z || !bias || !Qp || !idx || N <= 0 || ldz < 6 * E || ldq < E || (ldz % 4) || (ldq % 4)) return VQF_E_BADARG;
  if (!vqf_phrase_ngram_supported(T, E) || (long long)N * T * (E / 4) >= (1LL << 31)) return VQF_E_UNSUPPORTED;
  if (!aligned16(Z) || !aligned16(bias) || !aligned16(Qp) || (((uintptr_t)idx) & 3) || (((uintptr_t)lens) & 3)) return VQF_E_ALIGN;
  const long long n4 = (long long)N * T * (E / 4);
  VQF_LAUNCH(KID_PHRASE_FWD, phrase_ngram_fwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Z, ldz,
             bias, N * T, T, E, Qp, ldq, idx, lens);
  return vqf_last_error();
}

int phrase_bwd_launch(const float* dQp, int ldd, const float* Qp, int ldq, const uint8_t* idx, const int* lens, int N, int T, int E,
                      float* dZ, int ldz, void* stream) {
  if (!dQp || !Qp || !idx || !dZ || N <= 0 || ldz < 6 * E || ldq < E || ldd < E || (ldz % 4) || (ldq % 4) || (ldd % 4))
    return VQF_E_BADARG;
  if (!vqf_phrase_ngram_supported(T, E) || (long long)N * T * (E / 4) >= (1LL << 31)) return VQF_E_UNSUPPORTED;
  if (!aligned16(dQp) || !aligned16(Qp) || !aligned16(dZ) || (((uintptr_t)idx) & 3) || (((uintptr_t)lens) & 3)) return VQF_E_ALIGN;
  const long long n4 = (long long)N * T * (E / 4);
  VQF_LAUNCH(KID_PHRASE_BWD, phrase_ngram_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dQp,
             ldd, Qp, ldq, idx, N * T, T, E, dZ, ldz, lens);
  return vqf_last_error();
}

}  // namespace

extern "C" {

int vqf_phrase_ngram_supported(int T, int E) {
  return T >= 1 && T <= PH_TMAX && E >= 4 && (E % 4) == 0;
}

int vqf_phrase_ngram_fwd(const float* Z, int ldz, const float* bias, int N, int T, int E, float* Qp, int ldq, uint8_t* idx,
                         void* stream) {
  return phrase_fwd_launch(Z, ldz, bias, nullptr, N, T, E, Qp, ldq, idx, stream);
}

int vqf_phrase_ngram_bwd(const float* dQp, int ldd, const float* Qp, int ldq, const uint8_t* idx, int N, int T, int E, float* dZ,
                         int ldz, void* stream) {
  return phrase_bwd_launch(dQp, ldd, Qp, ldq, idx, nullptr, N, T, E, dZ, ldz, stream);
}

int vqf_phrase_ngram_fwd_len(const float* Z, int ldz, const float* bias, const int* lens, int N, int T, int E, float* Qp, int ldq,
                             uint8_t* idx, void* stream) {
  if (!lens) return VQF_E_BADARG;
  return phrase_fwd_launch(Z, ldz, bias, lens, N, T, E, Qp, ldq, idx, stream);
}

int vqf_phrase_ngram_bwd_len(const float* dQp, int ldd, const float* Qp, int ldq, const uint8_t* idx, const int* lens, int N, int T,
                             int E, float* dZ, int ldz, void* stream) {
  if (!lens) return VQF_E_BADARG;
  return phrase_bwd_launch(dQp, ldd, Qp, ldq, idx, lens, N, T, E, dZ, ldz, stream);
}

int vqf_tanh_bwd_rows_len(const float* dy, const float* y, const int* lens, int N, int T, int L, float* dx, void* stream) {
  if (!dy || !y || !lens || !dx || N <= 0 || T <= 0 || L <= 0) return VQF_E_BADARG;
  const long long n = (long long)N * T * L;
  if (n % 4) return VQF_E_UNSUPPORTED;
  if (!aligned16(dy) || !aligned16(y) || !aligned16(dx) || (((uintptr_t)lens) & 3)) return VQF_E_ALIGN;
  long long blocks = (n / 4 + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  VQF_LAUNCH(KID_TANH_DROP_BWD, tanh_bwd_rows_len_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dy, y, lens,
             n / 4, T, L, dx);
  return vqf_last_error();
}

}  // extern "C"
