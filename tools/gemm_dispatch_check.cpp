// Host-side check of the GEMM launchers (csrc/gemm_f32*.hip, gemm_bf16*.hip and the shared rules of csrc/gemm_host.h) under the
// host sanitizers: the routing queries of tests/test_gemm_entry_cpu.py over its grid of shapes and options, and refused calls of
// every GEMM entry point -- one valid-looking call per entry point (aligned fake addresses, never dereferenced; never made
// itself), broken in one way at a time and in pairs of those ways.  Each call returns before anything is launched, so this needs
// no GPU and must not run on one.  A fault carries its code and the place of its test in the entry point's order of refusals; a
// pair is refused by the one that is tested first.  Build the seven sources and this file with the host sanitizers, the rest of the
// library as it is, link them into one program, and run it (D: any scratch directory):
//   cd vqa-attention-networks_amd/csrc && make && G="gemm_f32 gemm_f32_big gemm_f32_wave gemm_f32_n80 gemm_f32_sample gemm_bf16 gemm_bf16_big"
//   for f in $G; do hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -c $f.hip -o $D/$f.san.o; done
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -I ../../include -c ../../tools/gemm_dispatch_check.cpp -o $D/check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $D/check.o $(for f in $G; do echo $D/$f.san.o; done) \
//         $(ls *.o | grep -v -E '^gemm_') -o $D/gemm_dispatch_check && $D/gemm_dispatch_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vqa_fusion.h"

static int failures = 0, calls = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    ++calls;                                                             \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static const long long FAKE = 1 << 20;                      // 16-byte aligned, never dereferenced
static float* fp(long long a) { return reinterpret_cast<float*>(static_cast<uintptr_t>(a)); }
static void* vp(long long a) { return reinterpret_cast<void*>(static_cast<uintptr_t>(a)); }
static const int Bad = VQF_E_BADARG, Ali = VQF_E_ALIGN, Uns = VQF_E_UNSUPPORTED;

struct Fault { const char* name; int i0; long long v0; int i1; long long v1; int code; int rank; };      // i1 < 0: one argument
typedef int (*Call)(const long long* a);

// every single fault, then every pair of faults that change different arguments
static void refusals(const char* entry, Call call, std::vector<long long> base, const std::vector<Fault>& faults) {
  auto apply = [](std::vector<long long>& a, const Fault& f) { a[f.i0] = f.v0; if (f.i1 >= 0) a[f.i1] = f.v1; };
  for (size_t i = 0; i < faults.size(); ++i) {
    std::vector<long long> a = base;
    apply(a, faults[i]);
    ++calls;
    const int got = call(a.data());
    if (got != faults[i].code) { std::printf("FAILED %s %s: %d\n", entry, faults[i].name, got); ++failures; }
    for (size_t j = i + 1; j < faults.size(); ++j) {
      const Fault &p = faults[i], &q = faults[j];
      if (p.i0 == q.i0 || p.i0 == q.i1 || (p.i1 >= 0 && (p.i1 == q.i0 || p.i1 == q.i1))) continue;
      std::vector<long long> b = a;
      apply(b, q);
      const int want = p.rank <= q.rank ? p.code : q.code;
      ++calls;
      const int rc = call(b.data());
      if (rc != want) { std::printf("FAILED %s %s&%s: %d\n", entry, p.name, q.name, rc); ++failures; }
    }
  }
}

// ---- the entry points over an argument array (the positions are those of include/vqa_fusion.h) ----------------------------------
#define I(k) static_cast<int>(a[k])
static int c_f32(const long long* a) {
  return vqf_gemm_f32(I(0), I(1), I(2), I(3), I(4), fp(a[5]), I(6), fp(a[7]), I(8), fp(a[9]), I(10), fp(a[11]), I(12), vp(a[13]), (size_t)a[14], vp(a[15]));
}
static int c_f32_rowscale(const long long* a) {
  return vqf_gemm_f32_rowscale(I(0), I(1), I(2), I(3), I(4), fp(a[5]), I(6), fp(a[7]), I(8), fp(a[9]), I(10), fp(a[11]), I(12), fp(a[13]), I(14), vp(a[15]));
}
static int c_f32_batched(const long long* a) {
  return vqf_gemm_f32_batched(I(0), I(1), I(2), I(3), I(4), I(5), fp(a[6]), I(7), a[8], fp(a[9]), I(10), a[11], fp(a[12]), I(13), a[14], I(15), vp(a[16]));
}
static int c_bf16(const long long* a) {
  return vqf_gemm_bf16(I(0), I(1), I(2), I(3), I(4), vp(a[5]), I(6), vp(a[7]), I(8), fp(a[9]), I(10), fp(a[11]), I(12), vp(a[13]), (size_t)a[14], vp(a[15]));
}
static int c_bf16_rowscale(const long long* a) {
  return vqf_gemm_bf16_rowscale(I(0), I(1), I(2), I(3), I(4), vp(a[5]), I(6), vp(a[7]), I(8), fp(a[9]), I(10), fp(a[11]), I(12), fp(a[13]), I(14), vp(a[15]));
}
static int c_sample(const long long* a) {
  return vqf_gemm_f32_sample(I(0), I(1), I(2), I(3), I(4), fp(a[5]), I(6), fp(a[7]), I(8), fp(a[9]), I(10), fp(a[11]), I(12), vp(a[13]));
}
static int c_lstm(const long long* a) {
  return vqf_lstm_step_fwd(fp(a[0]), fp(a[1]), fp(a[2]), fp(a[3]), I(4), I(5), fp(a[6]), fp(a[7]), vp(a[8]));
}
#undef I

struct Option { int id, value; };
struct WithOption {
  Option o; int prev = -1;
  explicit WithOption(Option opt) : o(opt) { if (o.id >= 0) vqf_set_option(o.id, o.value, &prev); }
  ~WithOption() { if (o.id >= 0) vqf_set_option(o.id, prev, nullptr); }
};

int main() {
  // ---- the queries: the grid of tests/test_gemm_entry_cpu.py, every (ta, tb), under the options that change the answers ---------
  static const int shapes[][3] = {
      {100352, 5000, 2048}, {5000, 2048, 100352}, {1024, 1024, 100352}, {4096, 1024, 7168}, {512, 5000, 2048}, {1024, 512, 50176},
      {50176, 512, 512}, {50176, 1024, 1024}, {8192, 8192, 1536}, {8192, 8192, 1532}, {7936, 8448, 1536}, {7936, 8448, 1532},
      {8192, 8192, 1024}, {5000, 2048, 16384}, {5000, 2048, 16380}, {4096, 1024, 4096}, {4096, 1024, 4092}, {4096, 1916, 7168},
      {4096, 1912, 7168}, {4096, 300, 7168}, {2048, 2048, 2048}, {1792, 2304, 2048}, {2048, 2048, 50176}, {1792, 2304, 50176},
      {2048, 1792, 50176}, {4098, 1024, 7168}, {4100, 1024, 7168}, {4096, 1026, 7168}, {4096, 1028, 7168}, {256, 128, 64},
      {255, 128, 64}, {256, 127, 64}, {256, 128, 60}, {256, 128, 255}, {64, 64, 64}};
  const Option none = {-1, 0}, options[] = {none, {VQF_OPT_GEMM_F32_BIG, 0}, {VQF_OPT_GEMM_F32_BIG, 2}, {VQF_OPT_GEMM_BF16_BIG, 0},
                                            {VQF_OPT_GEMM_F32_ROUNDS, 0}, {VQF_OPT_GEMM_F32_WAVE, 0}, {VQF_OPT_GEMM_F32_WAVE, 1}};
  for (const Option& o : options) {
    WithOption w(o);
    for (const auto& s : shapes)
      for (int t = 0; t < 4; ++t) {
        const int ta = t >> 1, tb = t & 1, M = s[0], N = s[1], K = s[2];
        const size_t slab = (size_t)M * N * sizeof(float);
        const size_t wf = vqf_gemm_f32_ws_bytes(ta, tb, M, N, K), wb = vqf_gemm_bf16_ws_bytes(ta, tb, M, N, K);
        const int rows = vqf_gemm_f32_big_rows(ta, tb, M, N, K);
        CHECK(wf % slab == 0 && wf / slab != 1 && wf / slab <= 32);          // no slabs, or 2 .. 32 of them
        CHECK(wb % slab == 0 && wb / slab != 1 && wb / slab <= 16);
        CHECK(rows == 0 || rows == M);                                       // (without a device no whole-rounds block)
        CHECK(wf == 0 || rows == M);                                         // slabs only where the large-tile kernel takes the product
        if (o.id == VQF_OPT_GEMM_F32_BIG && o.value == 0) CHECK(wf == 0 && rows == 0);
        if (o.id == VQF_OPT_GEMM_BF16_BIG && o.value == 0) CHECK(wb == 0);
        if (M < 256 || N < 128) CHECK(wf == 0 && wb == 0 && rows == 0);
      }
    for (int B : {0, 64, 128, 130, 256, 512})
      for (int H : {0, 128, 256, 264, 272, 512, 1024}) {
        const bool want = B > 0 && B % 128 == 0 && H >= 256 && H % 16 == 0 && !(o.id == VQF_OPT_GEMM_F32_WAVE && o.value == 0);
        CHECK((vqf_lstm_step_supported(B, H) != 0) == want);
      }
  }
  // the project's own shapes (tests/golden/gemm_entry.json)
  CHECK(vqf_gemm_f32_ws_bytes(0, 0, 100352, 5000, 2048) == 0 && vqf_gemm_f32_big_rows(0, 0, 100352, 5000, 2048) == 100352);
  CHECK(vqf_gemm_f32_ws_bytes(1, 1, 5000, 2048, 100352) == (size_t)8 * 5000 * 2048 * 4);
  CHECK(vqf_gemm_f32_ws_bytes(1, 1, 1024, 1024, 100352) == (size_t)16 * 1024 * 1024 * 4);
  CHECK(vqf_gemm_f32_ws_bytes(1, 1, 4096, 1024, 7168) == (size_t)4 * 4096 * 1024 * 4);
  CHECK(vqf_gemm_f32_ws_bytes(1, 1, 4096, 1024, 4092) == 0 && vqf_gemm_f32_ws_bytes(1, 1, 4096, 1912, 7168) == 0);
  CHECK(vqf_gemm_f32_big_rows(0, 0, 8192, 8192, 1536) == 8192 && vqf_gemm_f32_big_rows(0, 0, 8192, 8192, 1532) == 0);
  CHECK(vqf_gemm_bf16_ws_bytes(1, 1, 1792, 2304, 50176) == 0 && vqf_gemm_bf16_ws_bytes(1, 1, 2048, 2048, 50176) != 0);

  // ---- the refusals ------------------------------------------------------------------------------------------------------------
  // vqf_gemm_f32 and its kin: ta tb M N K A lda B ldb C ldc bias flags (ws ws_bytes | rowscale rows_per_scale) stream
  const std::vector<long long> gemm = {0, 0, 64, 64, 64, FAKE, 64, FAKE, 64, FAKE, 64, 0, 0, 0, 0, 0};
  std::vector<long long> scaled = gemm;
  scaled[13] = FAKE; scaled[14] = 4;
  const std::vector<Fault> bad = {{"A=0", 5, 0, -1, 0, Bad, 2}, {"B=0", 7, 0, -1, 0, Bad, 2}, {"C=0", 9, 0, -1, 0, Bad, 2},
                                  {"M=0", 2, 0, -1, 0, Bad, 2}, {"N=0", 3, 0, -1, 0, Bad, 2}, {"K=-1", 4, -1, -1, 0, Bad, 2},
                                  {"lda=0", 6, 0, -1, 0, Bad, 2}, {"ldb=-8", 8, -8, -1, 0, Bad, 2}, {"ldc=56", 10, 56, -1, 0, Bad, 2}};
  // the rowscale entries test rowscale / rows_per_scale first; the fp32 one then the other arguments and the flags last, the
  // bf16 one the flags BEFORE the other arguments
  const std::vector<Fault> scale = {{"rowscale=0", 13, 0, -1, 0, Bad, 0}, {"rows_per_scale=0", 14, 0, -1, 0, Bad, 0}};
  const std::vector<Fault> bf = {{"A+8", 5, FAKE + 8, -1, 0, Uns, 3}, {"B+2", 7, FAKE + 2, -1, 0, Uns, 3}, {"lda=68", 6, 68, -1, 0, Uns, 3},
                                 {"ldb=76", 8, 76, -1, 0, Uns, 3}, {"K=60", 4, 60, -1, 0, Uns, 3}, {"ta=1,K=60", 0, 1, 4, 60, Uns, 3},
                                 {"ta=1,M=60", 0, 1, 2, 60, Uns, 3}, {"ta=1,M=4", 0, 1, 2, 4, Uns, 3}, {"tb=1,N=60", 1, 1, 3, 60, Uns, 3}};
  auto join = [](std::vector<Fault> a, const std::vector<Fault>& b) { a.insert(a.end(), b.begin(), b.end()); return a; };
  refusals("vqf_gemm_f32", c_f32, gemm, bad);
  refusals("vqf_gemm_f32_rowscale", c_f32_rowscale, scaled,
           join(join(bad, scale), {{"flags=accum", 12, VQF_GEMM_ACCUM, -1, 0, Uns, 3}, {"flags=accum|relu", 12, 3, -1, 0, Uns, 3}}));
  refusals("vqf_gemm_bf16", c_bf16, gemm, join(join(bad, bf), {{"flags=out_bf16", 12, VQF_GEMM_OUT_BF16, -1, 0, Uns, 3}}));
  refusals("vqf_gemm_bf16_rowscale", c_bf16_rowscale, scaled,
           join(join(join(bad, bf), scale), {{"flags=accum", 12, VQF_GEMM_ACCUM, -1, 0, Uns, 1}, {"flags=out_bf16", 12, VQF_GEMM_OUT_BF16, -1, 0, Uns, 1}}));
  {   // ta tb batch M N K A lda strideA B ldb strideB C ldc strideC flags stream
    const std::vector<long long> b = {0, 0, 2, 64, 64, 64, FAKE, 64, 4096, FAKE, 64, 4096, FAKE, 64, 4096, 0, 0};
    refusals("vqf_gemm_f32_batched", c_f32_batched, b,
             {{"A=0", 6, 0, -1, 0, Bad, 0}, {"B=0", 9, 0, -1, 0, Bad, 0}, {"C=0", 12, 0, -1, 0, Bad, 0}, {"batch=0", 2, 0, -1, 0, Bad, 0},
              {"batch=65536", 2, 65536, -1, 0, Bad, 0}, {"M=0", 3, 0, -1, 0, Bad, 0}, {"N=0", 4, 0, -1, 0, Bad, 0}, {"K=-1", 5, -1, -1, 0, Bad, 0},
              {"lda=0", 7, 0, -1, 0, Bad, 0}, {"ldb=-8", 10, -8, -1, 0, Bad, 0}, {"ldc=56", 13, 56, -1, 0, Bad, 0}});
  }
  {   // tb NS L N K A lda B ldb C ldc bias flags stream: the arguments, then the shape, then the alignment.  The faults are those of
      // the pytest table but for the too-small leading dimensions: 40 here, 508 there.  508 is too small only beside K = N = 512, so a
      // pair with K=500 or N=300 is refused for the shape instead (the golden file records that); 40 stays a fault beside every other
      // one, which is what lets a pair's code follow from the two faults' places alone.
    const std::vector<long long> s = {0, 128, 196, 512, 512, FAKE, 512, FAKE, 512, FAKE, 512, 0, 0, 0};
    refusals("vqf_gemm_f32_sample", c_sample, s,
             {{"A=0", 5, 0, -1, 0, Bad, 0}, {"B=0", 7, 0, -1, 0, Bad, 0}, {"C=0", 9, 0, -1, 0, Bad, 0}, {"lda=40", 6, 40, -1, 0, Bad, 0},
              {"ldb=40", 8, 40, -1, 0, Bad, 0}, {"ldc=40", 10, 40, -1, 0, Bad, 0}, {"tb=1,ldb=40", 0, 1, 8, 40, Bad, 0}, {"NS=0", 1, 0, -1, 0, Uns, 1}, {"L=100", 2, 100, -1, 0, Uns, 1},
              {"L=198", 2, 198, -1, 0, Uns, 1}, {"L=204", 2, 204, -1, 0, Uns, 1}, {"N=300", 3, 300, -1, 0, Uns, 1}, {"K=48", 4, 48, -1, 0, Uns, 1},
              {"K=500", 4, 500, -1, 0, Uns, 1}, {"flags=accum", 12, VQF_GEMM_ACCUM, -1, 0, Uns, 1}, {"A+4", 5, FAKE + 4, -1, 0, Ali, 2},
              {"B+8", 7, FAKE + 8, -1, 0, Ali, 2}, {"C+4", 9, FAKE + 4, -1, 0, Ali, 2}, {"lda=514", 6, 514, -1, 0, Ali, 2},
              {"ldb=518", 8, 518, -1, 0, Ali, 2}, {"ldc=513", 10, 513, -1, 0, Ali, 2}});
  }
  {   // h_prev w_hh gates c_prev B H c_out h_out stream
    const std::vector<long long> l = {FAKE, FAKE, FAKE, FAKE, 128, 256, FAKE, FAKE, 0};
    refusals("vqf_lstm_step_fwd", c_lstm, l,
             {{"h_prev=0", 0, 0, -1, 0, Bad, 0}, {"w_hh=0", 1, 0, -1, 0, Bad, 0}, {"gates=0", 2, 0, -1, 0, Bad, 0}, {"c_out=0", 6, 0, -1, 0, Bad, 0},
              {"h_out=0", 7, 0, -1, 0, Bad, 0}, {"B=0", 4, 0, -1, 0, Bad, 0}, {"H=-16", 5, -16, -1, 0, Bad, 0}, {"B=100", 4, 100, -1, 0, Uns, 1},
              {"H=128", 5, 128, -1, 0, Uns, 1}, {"H=264", 5, 264, -1, 0, Uns, 1}, {"h_prev+4", 0, FAKE + 4, -1, 0, Ali, 2},
              {"w_hh+8", 1, FAKE + 8, -1, 0, Ali, 2}, {"gates+4", 2, FAKE + 4, -1, 0, Ali, 2}, {"c_prev+4", 3, FAKE + 4, -1, 0, Ali, 2},
              {"c_out+12", 6, FAKE + 12, -1, 0, Ali, 2}, {"h_out+4", 7, FAKE + 4, -1, 0, Ali, 2}});
  }
  if (failures) std::printf("%d of %d check(s) failed\n", failures, calls);
  else std::printf("gemm dispatch: all %d checks passed\n", calls);
  return failures ? 1 : 0;
}
