// What an operand from outside the vector register file costs a full-rate vector instruction on gfx950 — the forms design Q's step issues
// (csrc/sdrfm_q.hip, DESIGN.md 4.Q "operand forms"):
//   v_fma_f32 with three register operands | with one scalar-register operand | v_fmaak_f32 / v_fmamk_f32 (a 32-bit literal)
//   v_xor_b32 with a register operand | with a 32-bit literal
// each alone (15 instructions per loop pass over 8 independent destinations) and interleaved with v_smfmac_i32_16x16x128_i8 as the step has
// them (FILL = 4 and 8 vector instructions behind every matrix issue, as ubench13 does for v_xor), at 3 and 4 waves per SIMD.
// One workgroup of 256 threads = one wave per SIMD of a CU; 256 * waves-per-SIMD workgroups.  Prints one JSON line per measurement:
// ns per vector instruction and SIMD (alone), ns per matrix issue with its FILL vector instructions (interleaved).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)
typedef int i4 __attribute__((ext_vector_type(4)));
typedef int i8v __attribute__((ext_vector_type(8)));

enum { F_FMA_VVV = 0, F_FMA_S = 1, F_FMAAK = 2, F_FMAMK = 3, F_XOR_LIT = 4, F_XOR_V = 5, NFORM = 6 };
static const char* const kForm[NFORM] = {"v_fma_f32 v, v, v", "v_fma_f32 v, s, v", "v_fmaak_f32 (literal)", "v_fmamk_f32 (literal)", "v_xor_b32 literal", "v_xor_b32 v"};

template <int FORM>
__device__ __forceinline__ void one(float& d, float a, float kv, int ks) {
  // (every form: d <- f(d, ...) on one of 8 independent destinations; the multiplier keeps the values finite)
  if constexpr (FORM == F_FMA_VVV) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(kv));
  else if constexpr (FORM == F_FMA_S) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(d) : "v"(a), "s"(ks));
  else if constexpr (FORM == F_FMAAK) asm volatile("v_fmaak_f32 %0, %1, %0, 0x3a83126f" : "+v"(d) : "v"(a));
  else if constexpr (FORM == F_FMAMK) asm volatile("v_fmamk_f32 %0, %1, 0x3a83126f, %0" : "+v"(d) : "v"(a));
  else if constexpr (FORM == F_XOR_LIT) asm volatile("v_xor_b32 %0, 0x80808080, %0" : "+v"(d));
  else asm volatile("v_xor_b32 %0, %1, %0" : "+v"(d) : "v"(kv));
}

// FILL = 0: the form alone, 15 per pass.  FILL > 0: 15 matrix issues per pass, FILL instructions of the form behind each.
template <int FORM, int FILL>
__global__ void __launch_bounds__(256) k_rate(float* out, int iters, int seed) {
  i4 a = {seed * 3 + (int)threadIdx.x, seed, seed * 7, seed + 5};
  i8v b = {seed + 11, (int)threadIdx.x, seed * 5, seed * 13, seed, seed + 1, seed + 2, seed + 3};
  const int idx = (threadIdx.x & 1) ? 0xDDDDDDDD : 0x88888888;
  i4 acc[3] = {i4{0, 0, 0, 0}, i4{0, 0, 0, 0}, i4{0, 0, 0, 0}};
  float u[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) u[i] = 1.0f + 0.001f * (float)(threadIdx.x + i);
  float av = 0.5f, kv = (FORM == F_XOR_V) ? __builtin_bit_cast(float, 0x80808080u) : 0.001f;
  const int ks = 0x3a83126f;                                    // (0.001 in a scalar register: set once before the loop)
  asm volatile("" : "+v"(av), "+v"(kv));
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int m = 0; m < 15; ++m) {
      if constexpr (FILL == 0) {
        one<FORM>(u[m & 7], av, kv, ks);
      } else {
        asm volatile("v_smfmac_i32_16x16x128_i8 %0, %1, %2, %3" : "+v"(acc[m % 3]) : "v"(a), "v"(b), "v"(idx));
#pragma unroll
        for (int f = 0; f < FILL; ++f) one<FORM>(u[(m * FILL + f) & 7], av, kv, ks);
      }
    }
  }
  asm volatile("s_nop 15\n s_nop 15");
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) s += (float)(acc[i].x + acc[i].y + acc[i].z + acc[i].w);
#pragma unroll
  for (int i = 0; i < 8; ++i) s += u[i];
  if (s == 12345.678f) out[0] = s;
}

template <int FORM, int FILL>
static void run(float* d_out, int wps) {
  const int blocks = 256 * wps, iters = FILL ? 4000 : 20000;
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  k_rate<FORM, FILL><<<blocks, 256>>>(d_out, 500, 3);
  CK(hipDeviceSynchronize());
  float best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {                           // the best of three (a first launch may meet a lower clock)
    CK(hipEventRecord(e0));
    k_rate<FORM, FILL><<<blocks, 256>>>(d_out, iters, 3);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    if (ms < best) best = ms;
  }
  const double per = best * 1e6 / ((double)wps * iters * 15);   // ns per loop slot (one vector instruction, or one matrix issue with its FILL) and SIMD
  if (FILL) printf("{\"form\":\"%s\",\"per_smfmac\":%d,\"waves_per_simd\":%d,\"ns_per_smfmac_with_fill_per_simd\":%.3f}\n", kForm[FORM], FILL, wps, per);
  else printf("{\"form\":\"%s\",\"per_smfmac\":0,\"waves_per_simd\":%d,\"ns_per_instr_per_simd\":%.3f}\n", kForm[FORM], wps, per);
  fflush(stdout);
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
}

template <int FORM>
static void all_fills(float* d_out, int wps) {
  run<FORM, 0>(d_out, wps);
  run<FORM, 4>(d_out, wps);
  run<FORM, 8>(d_out, wps);
}

int main() {
  float* d_out; CK(hipMalloc(&d_out, 1024));
  for (int wps : {3, 4}) {
    all_fills<F_FMA_VVV>(d_out, wps);
    all_fills<F_FMA_S>(d_out, wps);
    all_fills<F_FMAAK>(d_out, wps);
    all_fills<F_FMAMK>(d_out, wps);
    all_fills<F_XOR_LIT>(d_out, wps);
    all_fills<F_XOR_V>(d_out, wps);
  }
  CK(hipFree(d_out));
  return 0;
}
