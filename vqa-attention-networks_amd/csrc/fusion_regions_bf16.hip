// The bf16 image projection on counted and packed regions (MFB / MHBCoAtt regions_bf16): the entry points of the image fusion with a
// bf16 P and / or a bf16 dP on the un-grouped region layouts, and the row-padding cast.  Argument checks only: the kernels and their
// launch functions are fusion.hip's (common.h: vqf_fuse_fwd_regions_bf16 / vqf_fuse_bwd_regions_bf16) and gemm_bf16.hip's cast; no
// kernel is launched from this file.
//
// The weight gradient dW = dP^T rows has K = the rows of dP, and the large-tile bf16 GEMM takes K % 32 == 0 only.  So the backward
// entry points take dP_rows >= the rows the kernels own (R packed, N*L counted) and leave rows R .. dP_rows - 1 of dP as exact zeros;
// the cast does the same for the other operand.  BOTH tails must be zeros: 0 * NaN from uninitialised memory is NaN.
// The _rb forwards (regions_bf16_coatt) leave the bf16 copy of R the same way: it is the other operand of co_att_conv1's weight gradient.
#include "common.h"

namespace {

// rows r0 .. r1 - 1 of a bf16 matrix with `ld` elements per row: +0.0 (at most a few rows: the K padding of the weight gradient)
int zero_rows_bf16(void* base, long long r0, long long r1, long long ld, void* stream) {
  if (r1 <= r0) return VQF_OK;
  const hipError_t e = hipMemsetAsync((char*)base + (size_t)r0 * ld * 2, 0, (size_t)(r1 - r0) * ld * 2, (hipStream_t)stream);
  return e == hipSuccess ? VQF_OK : (int)e;
}

// what every counted (lens) form refuses itself, in this order; rows = dP_rows, or N*L for a forward
int len_refusal(const int* lens, int N, int L, int O, long long rows) {
  if (!VqfRegions::ok(lens) || N <= 0 || L <= 0 || O <= 0) return VQF_E_BADARG;
  if (rows < (long long)N * L || rows >= (1LL << 31)) return VQF_E_BADARG;
  return (O % 4) ? VQF_E_UNSUPPORTED : VQF_OK;
}

// ... and every packed (roff) form; rows = dP_rows, or R for a forward
int packed_refusal(const int* roff, int N, int R, int L, int O, long long rows) {
  if (!VqfRegions::ok(roff) || R <= 0 || N <= 0 || L <= 0 || O <= 0) return VQF_E_BADARG;
  if (rows < R || rows >= (1LL << 31)) return VQF_E_BADARG;
  return vqf_mfb_fuse_packed_supported(N, N, R, L, O) ? VQF_OK : VQF_E_UNSUPPORTED;
}

// the bf16 copy of R of the _rb forms: given, 16-byte aligned, a pitch of at least O rounded up to 32 (the consumer GEMM's K padding;
// the kernel zeroes the pad columns up to the pitch, which fuse_fwd_impl bounds: ldrb % 4 == 0, ldrb <= 1024)
int rb_refusal(const void* R_bf16, int ldrb, int O) {
  if (!R_bf16 || ldrb < (O + 31) / 32 * 32) return VQF_E_BADARG;
  return aligned16(R_bf16) ? VQF_OK : VQF_E_ALIGN;
}

// the backward behind the checks: the zero tail first (the kernels never touch it), then the launch
int bwd_go(const float* dY, const float* Y, const float* inv, const float* coefA, const float* coefB, const void* P, int p_bf16,
           const float* pbias, const float* q, const uint8_t* keep, uint64_t seed, float p_drop, int N, int L, int O, void* dP,
           long long rows, int dP_rows, float* dq, float* dbiasP, void* ws, size_t ws_bytes, void* stream, const VqfRegions& rg) {
  if (!dP) return VQF_E_BADARG;
  if (!aligned16(dP)) return VQF_E_ALIGN;
  if (int rc = zero_rows_bf16(dP, rows, dP_rows, (long long)VQF_POOL_K * O, stream)) return rc;
  return vqf_fuse_bwd_regions_bf16(dY, Y, inv, coefA, coefB, P, p_bf16, pbias, q, keep, seed, p_drop, N, L, O, dP, dq, dbiasP, ws,
                                   ws_bytes, stream, rg);
}

}  // namespace

extern "C" {

int vqf_mfb_fuse_fwd_len_pbf16(const void* P_bf16, const float* pbias, const float* q, const int* lens, const uint8_t* keep,
                               uint64_t seed, float p_drop, int N, int L, int O, float* R, float* rowssq, void* stream) {
  const int rc = len_refusal(lens, N, L, O, (long long)N * L);
  return rc ? rc : vqf_fuse_fwd_regions_bf16(P_bf16, pbias, q, keep, seed, p_drop, N, L, O, R, rowssq, stream, {.lens = lens});
}

int vqf_mfb_fuse_fwd_packed_pbf16(const void* P_bf16, const float* pbias, const float* q, const int* roff, const uint8_t* keep,
                                  uint64_t seed, float p_drop, int N, int R, int L, int O, float* Rout, float* rowssq, void* stream) {
  const int rc = packed_refusal(roff, N, R, L, O, R);
  return rc ? rc
            : vqf_fuse_fwd_regions_bf16(P_bf16, pbias, q, keep, seed, p_drop, N, L, O, Rout, rowssq, stream, {.roff = roff, .Rtot = R});
}

int vqf_mfb_fuse_fwd_packed_rows_pbf16(const void* P_bf16, const float* pbias, const float* q, const int* roff, const uint8_t* keep,
                                       uint64_t seed, float p_drop, int N, int R, int L, int O, float* Rout, float* rowssq,
                                       void* stream) {
  const int rc = packed_refusal(roff, N, R, L, O, R);
  return rc ? rc
            : vqf_fuse_fwd_regions_bf16(P_bf16, pbias, q, keep, seed, p_drop, N, L, O, Rout, rowssq, stream,
                                        {.roff = roff, .Rtot = R, .rows = true});
}

// ... with the bf16 copy of R (the regions_bf16_coatt head's operand): R_bf16 (rb_rows, ldrb) in R's own rows, rb_rows >= rows.  The
// kernel writes rows 0 .. rows - 1 whole (pad columns and the rows behind a count as zeros); rows .. rb_rows - 1 are zeroed here, behind
// the launch, so that a refused call has touched nothing.
int vqf_mfb_fuse_fwd_len_pbf16_rb(const void* P_bf16, const float* pbias, const float* q, const int* lens, const uint8_t* keep,
                                  uint64_t seed, float p_drop, int N, int L, int O, float* R, void* R_bf16, int ldrb, int rb_rows,
                                  float* rowssq, void* stream) {
  int rc = len_refusal(lens, N, L, O, rb_rows);
  if (!rc) rc = rb_refusal(R_bf16, ldrb, O);
  if (!rc) rc = vqf_fuse_fwd_regions_bf16(P_bf16, pbias, q, keep, seed, p_drop, N, L, O, R, rowssq, stream, {.lens = lens}, R_bf16, ldrb);
  return rc ? rc : zero_rows_bf16(R_bf16, (long long)N * L, rb_rows, ldrb, stream);
}

int vqf_mfb_fuse_fwd_packed_pbf16_rb(const void* P_bf16, const float* pbias, const float* q, const int* roff, const uint8_t* keep,
                                     uint64_t seed, float p_drop, int N, int R, int L, int O, float* Rout, void* R_bf16, int ldrb,
                                     int rb_rows, float* rowssq, void* stream) {
  int rc = packed_refusal(roff, N, R, L, O, R);
  if (!rc && (long long)rb_rows < (long long)N * L) rc = VQF_E_BADARG;
  if (!rc) rc = rb_refusal(R_bf16, ldrb, O);
  if (!rc) rc = vqf_fuse_fwd_regions_bf16(P_bf16, pbias, q, keep, seed, p_drop, N, L, O, Rout, rowssq, stream,
                                          {.roff = roff, .Rtot = R}, R_bf16, ldrb);
  return rc ? rc : zero_rows_bf16(R_bf16, (long long)N * L, rb_rows, ldrb, stream);
}

int vqf_mfb_fuse_fwd_packed_rows_pbf16_rb(const void* P_bf16, const float* pbias, const float* q, const int* roff, const uint8_t* keep,
                                          uint64_t seed, float p_drop, int N, int R, int L, int O, float* Rout, void* R_bf16, int ldrb,
                                          int rb_rows, float* rowssq, void* stream) {
  int rc = packed_refusal(roff, N, R, L, O, rb_rows);
  if (!rc) rc = rb_refusal(R_bf16, ldrb, O);
  if (!rc) rc = vqf_fuse_fwd_regions_bf16(P_bf16, pbias, q, keep, seed, p_drop, N, L, O, Rout, rowssq, stream,
                                          {.roff = roff, .Rtot = R, .rows = true}, R_bf16, ldrb);
  return rc ? rc : zero_rows_bf16(R_bf16, R, rb_rows, ldrb, stream);
}

int vqf_mfb_fuse_bwd_len_pbf16(const float* dY, const float* Y, const float* inv, const float* coefA, const float* coefB,
                               const void* P_bf16, const float* pbias, const float* q, const int* lens, const uint8_t* keep,
                               uint64_t seed, float p_drop, int N, int L, int O, void* dP_bf16, int dP_rows, float* dq, float* dbiasP,
                               void* ws, size_t ws_bytes, void* stream) {
  const int rc = len_refusal(lens, N, L, O, dP_rows);
  return rc ? rc
            : bwd_go(dY, Y, inv, coefA, coefB, P_bf16, 1, pbias, q, keep, seed, p_drop, N, L, O, dP_bf16, (long long)N * L, dP_rows, dq,
                     dbiasP, ws, ws_bytes, stream, {.lens = lens});
}

int vqf_mfb_fuse_bwd_len_bf16dp(const float* dY, const float* Y, const float* inv, const float* coefA, const float* coefB,
                                const float* P, const float* pbias, const float* q, const int* lens, const uint8_t* keep, uint64_t seed,
                                float p_drop, int N, int L, int O, void* dP_bf16, int dP_rows, float* dq, float* dbiasP, void* ws,
                                size_t ws_bytes, void* stream) {
  const int rc = len_refusal(lens, N, L, O, dP_rows);
  return rc ? rc
            : bwd_go(dY, Y, inv, coefA, coefB, P, 0, pbias, q, keep, seed, p_drop, N, L, O, dP_bf16, (long long)N * L, dP_rows, dq,
                     dbiasP, ws, ws_bytes, stream, {.lens = lens});
}

int vqf_mfb_fuse_bwd_packed_pbf16(const float* dY, const float* Y, const float* inv, const float* coefA, const float* coefB,
                                  const void* P_bf16, const float* pbias, const float* q, const int* roff, const uint8_t* keep,
                                  uint64_t seed, float p_drop, int N, int R, int L, int O, void* dP_bf16, int dP_rows, float* dq,
                                  float* dbiasP, void* ws, size_t ws_bytes, void* stream) {
  const int rc = packed_refusal(roff, N, R, L, O, dP_rows);
  return rc ? rc
            : bwd_go(dY, Y, inv, coefA, coefB, P_bf16, 1, pbias, q, keep, seed, p_drop, N, L, O, dP_bf16, R, dP_rows, dq, dbiasP, ws,
                     ws_bytes, stream, {.roff = roff, .Rtot = R});
}

int vqf_mfb_fuse_bwd_packed_bf16dp(const float* dY, const float* Y, const float* inv, const float* coefA, const float* coefB,
                                   const float* P, const float* pbias, const float* q, const int* roff, const uint8_t* keep,
                                   uint64_t seed, float p_drop, int N, int R, int L, int O, void* dP_bf16, int dP_rows, float* dq,
                                   float* dbiasP, void* ws, size_t ws_bytes, void* stream) {
  const int rc = packed_refusal(roff, N, R, L, O, dP_rows);
  return rc ? rc
            : bwd_go(dY, Y, inv, coefA, coefB, P, 0, pbias, q, keep, seed, p_drop, N, L, O, dP_bf16, R, dP_rows, dq, dbiasP, ws,
                     ws_bytes, stream, {.roff = roff, .Rtot = R});
}

int vqf_mfb_fuse_bwd_packed_rows_pbf16(const float* dY, const float* Y, const float* inv, const float* coefA, const float* coefB,
                                       const void* P_bf16, const float* pbias, const float* q, const int* roff, const uint8_t* keep,
                                       uint64_t seed, float p_drop, int N, int R, int L, int O, void* dP_bf16, int dP_rows, float* dq,
                                       float* dbiasP, void* ws, size_t ws_bytes, void* stream) {
  const int rc = packed_refusal(roff, N, R, L, O, dP_rows);
  return rc ? rc
            : bwd_go(dY, Y, inv, coefA, coefB, P_bf16, 1, pbias, q, keep, seed, p_drop, N, L, O, dP_bf16, R, dP_rows, dq, dbiasP, ws,
                     ws_bytes, stream, {.roff = roff, .Rtot = R, .rows = true});
}

int vqf_mfb_fuse_bwd_packed_rows_bf16dp(const float* dY, const float* Y, const float* inv, const float* coefA, const float* coefB,
                                        const float* P, const float* pbias, const float* q, const int* roff, const uint8_t* keep,
                                        uint64_t seed, float p_drop, int N, int R, int L, int O, void* dP_bf16, int dP_rows, float* dq,
                                        float* dbiasP, void* ws, size_t ws_bytes, void* stream) {
  const int rc = packed_refusal(roff, N, R, L, O, dP_rows);
  return rc ? rc
            : bwd_go(dY, Y, inv, coefA, coefB, P, 0, pbias, q, keep, seed, p_drop, N, L, O, dP_bf16, R, dP_rows, dq, dbiasP, ws,
                     ws_bytes, stream, {.roff = roff, .Rtot = R, .rows = true});
}

int vqf_cast_f32_bf16_rows(const float* x, int R, int C, int ldx, void* y, int ldy, int y_rows, void* stream) {
  if (y_rows < R) return VQF_E_BADARG;
  const int rc = vqf_cast_f32_bf16(x, R, C, ldx, y, ldy, stream);
  return rc ? rc : zero_rows_bf16(y, R, y_rows, ldy, stream);
}

}  // extern "C"
