// Input staging: the reference's loader reads one .npy per image laid out
// [2048, 14, 14] (channels outermost) and turns it into the (196, 2048) region-major matrix on the
// CPU (data_loader.py:30-32: np.transpose(x, (1,2,0)).reshape(-1, 2048)).  Here the file bytes go
// to the GPU as they are and the batch is transposed on the way into its HBM-resident slot,
// optionally narrowing to bf16 (half the image traffic of every later pass).
//
// HBM-bound: 4 B read + 4 B (2 B) written per element; 64x64 tiles through LDS so that both the
// reads (along L) and the writes (along D) are contiguous 16-byte accesses.
#include "common.h"

namespace {

constexpr int TS = 64;            // tile edge
constexpr int TPAD = TS + 1;      // LDS row pitch (floats): column reads hit distinct banks

// src (N, D, L) fp32 -> dst (N, L, D) fp32 | bf16.   grid (ceil(L/64), ceil(D/64), N), 256 threads
template <bool BF16>
__global__ __launch_bounds__(256) void feat_transpose_kernel(const float* __restrict__ src, int D, int L,
                                                             void* __restrict__ dst_) {
  __shared__ float tile[TS * TPAD];            // tile[d][l]
  const int l0 = blockIdx.x * TS, d0 = blockIdx.y * TS;
  const size_t img = (size_t)blockIdx.z * D * L;
  const int tid = threadIdx.x;
  const float* s = src + img;
  const bool vec_in = ((L & 3) == 0) && aligned16_dev(src);

  // ---- read: 64 d-rows x 16 float4 along l
  {
    const int c4 = (tid & 15) * 4;                       // l offset within the tile
    for (int r = tid >> 4; r < TS; r += 16) {            // d row within the tile
      const int d = d0 + r, l = l0 + c4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (d < D) {
        if (vec_in && l + 3 < L) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(s + (size_t)d * L + l);
          v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (l + j < L) v[j] = s[(size_t)d * L + l + j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[r * TPAD + c4 + j] = v[j];
    }
  }
  __syncthreads();

  // ---- write: 64 l-rows x 16 groups of 4 consecutive d
  const int g4 = (tid & 15) * 4;                         // d offset within the tile
  const bool vec_out = ((D & 3) == 0) && aligned16_dev(dst_);
  for (int r = tid >> 4; r < TS; r += 16) {              // l row within the tile
    const int l = l0 + r, d = d0 + g4;
    if (l >= L || d >= D) continue;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = tile[(g4 + j) * TPAD + r];
    const size_t o = img + (size_t)l * D + d;
    if constexpr (BF16) {
      __bf16* dst = reinterpret_cast<__bf16*>(dst_);
      if (vec_out && d + 3 < D) {
        __bf16 h[4] = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        *reinterpret_cast<uint2*>(dst + o) = *reinterpret_cast<const uint2*>(h);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (d + j < D) dst[o + j] = (__bf16)v[j];
      }
    } else {
      float* dst = reinterpret_cast<float*>(dst_);
      if (vec_out && d + 3 < D) {
        f32x4 t = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(dst + o) = t;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (d + j < D) dst[o + j] = v[j];
      }
    }
  }
}

// Packed region features (detector boxes, never padded) as the H2D copy left them -> the fp32 tensors the models take.
// src (Rtot, D) fp32 | IEEE fp16 holds the real rows of every image, one image after the other.  HBM-bound, one pass: per lane one
// 16-byte (fp32) or 8-byte (fp16) streaming load and one 16-byte streaming store.  The fp16 widening is v_cvt_f32_f16: exact for
// every finite value, +-0, +-inf and -- the default kernel mode keeps fp16 subnormals -- the subnormals.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

template <bool F16>
__device__ __forceinline__ f32x4 stage_load4(const void* __restrict__ src, long long i4) {
  if constexpr (F16) {
    const f16x4 h = vqf_ld_stream(reinterpret_cast<const f16x4*>(src) + i4);
    return __builtin_convertvector(h, f32x4);
  } else {
    return vqf_ld_stream(reinterpret_cast<const f32x4*>(src) + i4);
  }
}

// packed output: dst (Rtot, D) = the same rows, widened.  n4 = Rtot * D / 4 < 2^43
template <bool F16>
__global__ void __launch_bounds__(256)
region_rows_widen_kernel(const void* __restrict__ src, long long n4, float* __restrict__ dst) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
    vqf_st_stream(reinterpret_cast<f32x4*>(dst) + i, stage_load4<F16>(src, i));
}

// padded output: dst (U*L, D); image u = blockIdx.y has (start, cnt) by vqf_packed_span's rule (common.h), read once per
// workgroup.  Row u*L + l is source row start + l for l < cnt and an exact +0.0 row behind it (nothing read there).
template <bool F16>
__global__ void __launch_bounds__(256)
region_rows_pad_kernel(const void* __restrict__ src, const int* __restrict__ roff, int Rtot, int L, int D4,
                       float* __restrict__ dst) {
  const int u = blockIdx.y;
  long long start;
  int cnt;
  vqf_packed_span(roff, u, L, Rtot, start, cnt);
  const unsigned n4 = (unsigned)L * (unsigned)D4;            // <= 2^24
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const unsigned l = i / (unsigned)D4, c4 = i - l * (unsigned)D4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((int)l < cnt) v = stage_load4<F16>(src, (start + l) * D4 + c4);
    vqf_st_stream(reinterpret_cast<f32x4*>(dst) + ((long long)u * L + l) * D4 + c4, v);
  }
}

}  // namespace

extern "C" int vqf_feat_transpose(const float* src, int N, int D, int L, int out_bf16, void* dst, void* stream) {
  if (!src || !dst || N <= 0 || D <= 0 || L <= 0) return VQF_E_BADARG;
  if (N > 65535 || (D + TS - 1) / TS > 65535) return VQF_E_UNSUPPORTED;
  dim3 grid((L + TS - 1) / TS, (D + TS - 1) / TS, N);
  hipStream_t s = (hipStream_t)stream;
  vqf_prof_dims(N, D, L);
  if (out_bf16)
    VQF_LAUNCH(KID_FEAT_TRANSPOSE, feat_transpose_kernel<true>, grid, dim3(256), 0, s, src, D, L, dst);
  else
    VQF_LAUNCH(KID_FEAT_TRANSPOSE, feat_transpose_kernel<false>, grid, dim3(256), 0, s, src, D, L, dst);
  return vqf_last_error();
}

extern "C" int vqf_region_rows_stage(const void* src, int src_f16, const int* roff, int U, int R, int L, int D, float* dst,
                                     void* stream) {
  if (!src || !dst || (roff && (((uintptr_t)roff) & 3)) || U <= 0 || R <= 0 || L <= 0 || D <= 0) return VQF_E_BADARG;
  if (U > 65535 || R >= (1 << 29) || L > 1024 || D < 4 || D > 65536 || (D % 4)) return VQF_E_UNSUPPORTED;
  if (!aligned16(dst) || (src_f16 ? (((uintptr_t)src) & 7) != 0 : !aligned16(src))) return VQF_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int D4 = D / 4;
  if (!roff) {
    const long long n4 = (long long)R * D4;
    long long blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    vqf_prof_dims(R, D, 0);
    if (src_f16)
      VQF_LAUNCH(KID_REGION_ROWS_STAGE, region_rows_widen_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, src, n4, dst);
    else
      VQF_LAUNCH(KID_REGION_ROWS_STAGE, region_rows_widen_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, src, n4, dst);
    return vqf_last_error();
  }
  int chunks = (L * D4 + 255) / 256;                         // L * D / 4 <= 2^24
  if (chunks > 64) chunks = 64;
  vqf_prof_dims(U, L, D);
  if (src_f16)
    VQF_LAUNCH(KID_REGION_ROWS_STAGE, region_rows_pad_kernel<true>, dim3((unsigned)chunks, (unsigned)U), dim3(256), 0, s, src, roff,
               R, L, D4, dst);
  else
    VQF_LAUNCH(KID_REGION_ROWS_STAGE, region_rows_pad_kernel<false>, dim3((unsigned)chunks, (unsigned)U), dim3(256), 0, s, src, roff,
               R, L, D4, dst);
  return vqf_last_error();
}
