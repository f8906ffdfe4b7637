// Probe of v_mfma_f32_16x16x128_f8f6f4 on gfx950: (1) numerics with the operand layout the 8-bit GEMM uses — lane l supplies row
// l % 16 and 32 consecutive bytes (k = 32 (l / 16) .. + 32) of a 128-k row, A and B alike (any k permutation is fine as long as both
// operands share it); e4m3 x e4m3 and e5m2 x e4m3; (2) issue rate against v_mfma_f32_16x16x32_bf16 (cycles per instruction with 16
// independent accumulators); (3) the precision of one instruction, for the error model of tests/fp8_reference.py: worst
// |D - fp64| / max_k |a_k b_k| of v_mfma_f32_16x16x128_f8f6f4 (128 k) and v_mfma_f32_16x16x32_{fp8,bf8}_fp8 (32 k), A e4m3 and e5m2,
// over operands at the GEMM test matrix's distribution, over bytes drawn from the whole finite code range, and over a staircase
// of equal-signed products 2^-s below the largest one; always against this file's own fp64 sum.  hipcc --offload-arch=gfx950 -O3 tools/probes/mfma_f8_probe.hip -o /tmp/mfma_f8_probe && /tmp/mfma_f8_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

template <int FA>
__global__ void mm(const uint8_t* a, const uint8_t* b, float* d) {
  const int lane = threadIdx.x;
  const i32x8 fa = *(const i32x8*)(a + (lane & 15) * 128 + (lane >> 4) * 32);
  const i32x8 fb = *(const i32x8*)(b + (lane & 15) * 128 + (lane >> 4) * 32);
  f32x4 c = {0, 0, 0, 0};
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa, fb, c, FA, 0, 0, 0, 0, 0);
  // D[i][j]: lane holds column j = lane % 16 (row of B), rows i = 4 (lane / 16) + r (rows of A)
  for (int r = 0; r < 4; ++r) d[(4 * (lane >> 4) + r) * 16 + (lane & 15)] = c[r];
}

// one instruction per block, blockIdx.x-th operand set; c0: the accumulator going in (NULL: 0)
template <int FA>
__global__ void mm128b(const uint8_t* a, const uint8_t* b, const float* c0, float* d) {
  const int lane = threadIdx.x;
  a += (size_t)blockIdx.x * 2048; b += (size_t)blockIdx.x * 2048; d += (size_t)blockIdx.x * 256;
  const i32x8 fa = *(const i32x8*)(a + (lane & 15) * 128 + (lane >> 4) * 32);
  const i32x8 fb = *(const i32x8*)(b + (lane & 15) * 128 + (lane >> 4) * 32);
  f32x4 c = {0, 0, 0, 0};
  if (c0) for (int r = 0; r < 4; ++r) c[r] = c0[(size_t)blockIdx.x * 256 + (4 * (lane >> 4) + r) * 16 + (lane & 15)];
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa, fb, c, FA, 0, 0, 0, 0, 0);
  for (int r = 0; r < 4; ++r) d[(4 * (lane >> 4) + r) * 16 + (lane & 15)] = c[r];
}

// the 16x16x32 form as the 8-wave GEMM issues it: the e4m3 weight operand first, the activation (e4m3 / e5m2) second; lane l
// supplies row l % 16 and the 8 bytes k = 8 (l / 16) .. + 8 of a 32-k row.  Stored as D[activation row][weight row].
template <int FA>
__global__ void mm32b(const uint8_t* a, const uint8_t* b, const float* c0, float* d) {
  const int lane = threadIdx.x;
  a += (size_t)blockIdx.x * 512; b += (size_t)blockIdx.x * 512; d += (size_t)blockIdx.x * 256;
  const long x = *(const long*)(a + (lane & 15) * 32 + (lane >> 4) * 8);
  const long w = *(const long*)(b + (lane & 15) * 32 + (lane >> 4) * 8);
  f32x4 c = {0, 0, 0, 0};
  // D'[i][j]: i = 4 (lane / 16) + r a row of the FIRST operand (w), j = lane % 16 a row of the second (x)
  if (c0) for (int r = 0; r < 4; ++r) c[r] = c0[(size_t)blockIdx.x * 256 + (lane & 15) * 16 + 4 * (lane >> 4) + r];
  if constexpr (FA) c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_bf8(w, x, c, 0, 0, 0);
  else c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(w, x, c, 0, 0, 0);
  for (int r = 0; r < 4; ++r) d[(lane & 15) * 16 + 4 * (lane >> 4) + r] = c[r];
}

template <bool F8>
__global__ void rate(float* out, unsigned long long* cyc, int iters) {
  f32x4 acc[16];
  for (int i = 0; i < 16; ++i) acc[i] = f32x4{0, 0, 0, 0};
  i32x8 a8 = {1, 2, 3, 4, 5, 6, 7, 8}, b8 = {8, 7, 6, 5, 4, 3, 2, 1};
  bf16x8 a2, b2;
  for (int i = 0; i < 8; ++i) { a2[i] = (__bf16)(float)(threadIdx.x + i); b2[i] = (__bf16)(float)(i); }
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if constexpr (F8) acc[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, acc[i], 0, 0, 0, 0, 0, 0);
      else acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b2, acc[i], 0, 0, 0);
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  float s = 0;
  for (int i = 0; i < 16; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if (threadIdx.x == 0 && blockIdx.x == 0) *cyc = t1 - t0;
}

static float dec(uint8_t v, int e5m2) {
  const int s = v >> 7;
  float r;
  if (!e5m2) { const int e = (v >> 3) & 15, m = v & 7; r = e == 0 ? ldexpf((float)m, -9) : ldexpf(1.0f + m / 8.0f, e - 7); }
  else { const int e = (v >> 2) & 31, m = v & 3; r = e == 0 ? ldexpf((float)m, -16) : ldexpf(1.0f + m / 4.0f, e - 15); }
  return s ? -r : r;
}

static bool finite_code(uint8_t v, int e5m2) { return e5m2 ? ((v >> 2) & 31) != 31 : (v & 0x7f) != 0x7f; }

// nearest code of the format (ties: even code), saturating; host-side, by search over the 127 positive finite codes
static uint8_t enc(double x, int e5m2) {
  const uint8_t s = x < 0 ? 0x80 : 0;
  const double ax = fabs(x);
  int best = 0; double bd = ax;
  for (int c = 1; c < 128; ++c) {
    if (!finite_code((uint8_t)c, e5m2)) break;
    const double dd = fabs(ax - (double)dec((uint8_t)c, e5m2));
    if (dd < bd || (dd == bd && !(c & 1))) { bd = dd; best = c; }
  }
  return (uint8_t)(s | best);
}

static double urand() { return (rand() + 0.5) / ((double)RAND_MAX + 1.0) * 2.0 - 1.0; }

// precision of one instruction: NB operand sets of KK = 128 or 32 k; pattern 0: the GEMM test matrix's operands (uniform(-1, 1)
// quantised with the tensor-max scale, either format), 1: bytes uniform over all finite codes (every exponent of the format),
// 2: staircase (k = 0 the largest product, all others equal-signed and 2^-(i + j)-ish below it, full mantissas), 3: pattern 0
// with an accumulator of the size a running GEMM sum has.  Prints worst |D - fp64| / max_k |a_k b_k| (pattern 3: the fp32
// rounding of the accumulate, 2 u (|C| + sum |a b|), is taken off first: gemm_reference's delta_acc already holds it).
template <int KK, int FA>
static double precision(int pattern, int NB) {
  const size_t na = (size_t)NB * 16 * KK;
  uint8_t* ha = (uint8_t*)malloc(na); uint8_t* hb = (uint8_t*)malloc(na);
  float* hc = (float*)calloc((size_t)NB * 256, 4); float* hd = (float*)malloc((size_t)NB * 256 * 4);
  const double fmax_a = FA ? 57344.0 : 448.0;
  srand(1000 + 10 * pattern + FA + KK);
  for (int n = 0; n < NB; ++n)
    for (int i = 0; i < 16; ++i)
      for (int k = 0; k < KK; ++k) {
        const size_t o = ((size_t)n * 16 + i) * KK + k;
        if (pattern == 0 || pattern == 3) { ha[o] = enc(urand() * fmax_a, FA); hb[o] = enc(urand() * 448.0, 0); }
        else if (pattern == 1) {
          do ha[o] = (uint8_t)(rand() & 255); while (!finite_code(ha[o], FA));
          do hb[o] = (uint8_t)(rand() & 255); while (!finite_code(hb[o], 0));
        } else {
          const int sh = i < 14 ? i : 14;                 // e4m3: 2^8 .. 1.875 2^-6; e5m2: 2^15 .. 1.75 2^-13
          const int sign = (n & 1) ? 0x80 : 0;            // odd sets: the small products oppose the large one
          ha[o] = k == 0 ? enc(FA ? 32768.0 : 256.0, FA) : (uint8_t)(sign | enc(FA ? ldexp(1.75, 15 - 2 * sh) : ldexp(1.875, 8 - sh), FA));
          hb[o] = k == 0 ? enc(256.0, 0) : enc(ldexp(1.875, 8 - sh - (n >> 1) % 2), 0);
        }
      }
  if (pattern == 3)
    for (size_t o = 0; o < (size_t)NB * 256; ++o) hc[o] = (float)(urand() * fmax_a * 448.0 * 0.33 * sqrt(768.0));   // ~ a K = 768 sum
  uint8_t *a, *b; float *c, *d;
  hipMalloc(&a, na); hipMalloc(&b, na); hipMalloc(&c, (size_t)NB * 1024); hipMalloc(&d, (size_t)NB * 1024);
  hipMemcpy(a, ha, na, hipMemcpyHostToDevice); hipMemcpy(b, hb, na, hipMemcpyHostToDevice);
  hipMemcpy(c, hc, (size_t)NB * 1024, hipMemcpyHostToDevice);
  const float* c0 = pattern == 3 ? c : nullptr;
  if constexpr (KK == 128) hipLaunchKernelGGL((mm128b<FA>), NB, 64, 0, 0, a, b, c0, d);
  else hipLaunchKernelGGL((mm32b<FA>), NB, 64, 0, 0, a, b, c0, d);
  if (hipMemcpy(hd, d, (size_t)NB * 1024, hipMemcpyDeviceToHost) != hipSuccess) { printf("precision probe: launch failed\n"); exit(2); }
  double worst = 0, worst_of_sum = 0;
  for (int n = 0; n < NB; ++n)
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        double ref = hc[(size_t)n * 256 + i * 16 + j], mx = 0, sabs = fabs(ref);
        for (int k = 0; k < KK; ++k) {
          const double pr = (double)dec(ha[((size_t)n * 16 + i) * KK + k], FA) * (double)dec(hb[((size_t)n * 16 + j) * KK + k], 0);
          ref += pr; sabs += fabs(pr); mx = fmax(mx, fabs(pr));
        }
        if (mx == 0) continue;
        double err = fabs(ref - (double)hd[(size_t)n * 256 + i * 16 + j]);
        if (pattern == 3) err = fmax(0.0, err - ldexp(sabs, -23));
        worst = fmax(worst, err / mx);
        worst_of_sum = fmax(worst_of_sum, err / sabs);
      }
  static const char* names[] = {"matrix distribution", "whole code range", "staircase", "matrix distribution + accumulator"};
  printf("precision 16x16x%-3d A %s, %-33s: worst |D - fp64| / max_k|a_k b_k| = %.4e   (/ sum_k|a_k b_k| = %.3e; %d instructions)\n",
         KK, FA ? "e5m2" : "e4m3", names[pattern], worst, worst_of_sum, NB * 256);
  hipFree(a); hipFree(b); hipFree(c); hipFree(d); free(ha); free(hb); free(hc); free(hd);
  return worst;
}

int main() {
  uint8_t ha[16 * 128], hb[16 * 128];
  float hd[256];
  uint8_t *a, *b; float* d;
  hipMalloc(&a, sizeof ha); hipMalloc(&b, sizeof hb); hipMalloc(&d, sizeof hd);
  int bad = 0;
  for (int fa = 0; fa < 2; ++fa) {
    srand(7 + fa);
    for (int i = 0; i < 16 * 128; ++i) {
      // finite, moderate magnitudes: e4m3 exponent 4..9, e5m2 exponent 12..17
      ha[i] = fa ? (uint8_t)(((rand() & 1) << 7) | ((12 + rand() % 6) << 2) | (rand() & 3)) : (uint8_t)(((rand() & 1) << 7) | ((4 + rand() % 6) << 3) | (rand() & 7));
      hb[i] = (uint8_t)(((rand() & 1) << 7) | ((4 + rand() % 6) << 3) | (rand() & 7));
    }
    hipMemcpy(a, ha, sizeof ha, hipMemcpyHostToDevice); hipMemcpy(b, hb, sizeof hb, hipMemcpyHostToDevice);
    if (fa) hipLaunchKernelGGL(mm<1>, 1, 64, 0, 0, a, b, d); else hipLaunchKernelGGL(mm<0>, 1, 64, 0, 0, a, b, d);
    hipMemcpy(hd, d, sizeof hd, hipMemcpyDeviceToHost);
    double worst = 0;
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        double ref = 0;
        for (int k = 0; k < 128; ++k) ref += (double)dec(ha[i * 128 + k], fa) * (double)dec(hb[j * 128 + k], 0);
        const double err = fabs(ref - hd[i * 16 + j]) / (fabs(ref) + 1.0);
        if (err > worst) worst = err;
      }
    printf("A %s x B e4m3: worst relative error %.3g %s\n", fa ? "e5m2" : "e4m3", worst, worst < 1e-5 ? "ok" : "MISMATCH");
    for (int j = 0; j < 4; ++j) {
      double ref = 0, ref32 = 0; float f = 0;
      for (int k = 0; k < 128; ++k) { const float pr = dec(ha[k], fa) * dec(hb[j * 128 + k], 0); ref += pr; f += pr; }
      printf("   D[0][%d] = %.6f   fp64 reference %.6f   fp32 sequential %.6f\n", j, hd[j], ref, (double)f);
    }
    bad |= !(worst < 1e-5);
  }
  {   // small integers: every partial sum is exact in fp32 whatever the order — separates layout from accumulation precision
    srand(11);
    for (int i = 0; i < 16 * 128; ++i) {
      ha[i] = (uint8_t)(((rand() & 1) << 7) | ((7 + rand() % 2) << 3) | ((rand() & 3) << 1));   // +-{1, 1.25, 1.5, 1.75, 2, 2.5, 3, 3.5}
      hb[i] = (uint8_t)(((rand() & 1) << 7) | ((7 + rand() % 2) << 3) | ((rand() & 3) << 1));
    }
    hipMemcpy(a, ha, sizeof ha, hipMemcpyHostToDevice); hipMemcpy(b, hb, sizeof hb, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(mm<0>, 1, 64, 0, 0, a, b, d);
    hipMemcpy(hd, d, sizeof hd, hipMemcpyDeviceToHost);
    double worst = 0;
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        double ref = 0;
        for (int k = 0; k < 128; ++k) ref += (double)dec(ha[i * 128 + k], 0) * (double)dec(hb[j * 128 + k], 0);
        worst = fmax(worst, fabs(ref - hd[i * 16 + j]));
      }
    printf("quarter-integer operands (exact sums): worst absolute error %.3g\n", worst);
  }
  {   // the constants of tests/fp8_reference.py: c = 2 x the worst of these lines, per instruction form
    double w128 = 0, w32 = 0;
    for (int pat = 0; pat < 4; ++pat) {
      const int nb = pat == 2 ? 4 : 2048;
      w128 = fmax(w128, fmax(precision<128, 0>(pat, nb), precision<128, 1>(pat, nb)));
      w32 = fmax(w32, fmax(precision<32, 0>(pat, nb), precision<32, 1>(pat, nb)));
    }
    printf("worst over all patterns: 16x16x128 %.4e, 16x16x32 %.4e\n", w128, w32);
  }
  float* out; unsigned long long* cyc; unsigned long long hc;
  hipMalloc(&out, 256 * 4 * 1024); hipMalloc(&cyc, 8);
  for (int f8 = 0; f8 < 2; ++f8)
    for (int rep = 0; rep < 2; ++rep) {
      if (f8) hipLaunchKernelGGL(rate<true>, 1, 256, 0, 0, out, cyc, 2000); else hipLaunchKernelGGL(rate<false>, 1, 256, 0, 0, out, cyc, 2000);
      hipMemcpy(&hc, cyc, 8, hipMemcpyDeviceToHost);
      // s_memtime ticks at the constant 100 MHz reference: report ticks per instruction and let the ratio speak
      if (rep) printf("%s: %.4f reference ticks per MFMA (one wave per SIMD, 16 accumulators)\n", f8 ? "f8 16x16x128" : "bf16 16x16x32", (double)hc / (2000.0 * 16));
    }
  return bad;
}
