// linear_mac.hip -- the two multiply sequences of tlwe_linear_kernel (mosfhet_amd/csrc/linear_kernels.h: linear_mac<true> narrow, linear_mac<false> wide) ALONE:
// the dense walk's inner step -- one word per lane into TJ = 8 accumulators, the 8 weights of the step by one scalar load from a table that stays in the caches --
// with the words held in registers instead of loaded from memory.  What it prints is the rate the vector unit sustains on the sequence as the compiler writes
// it, the yardstick for the multiplies per second of the real call (tools/gpu_perf_tlwe_linear.py --modes ubench runs it).
// Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/ubench/linear_mac tools/ubench/linear_mac.hip      Run on the GPU box: tools/ubench/linear_mac
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "../../mosfhet_amd/csrc/linear_kernels.h"

using namespace mosfhet;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int WORDS = 16, STEPS = 64;   // words per lane held in registers; weight table [STEPS][WORDS][TJ]

template <bool NARROW>
__global__ __launch_bounds__(256) void mac_kernel(uint64_t *__restrict__ out, const int64_t *__restrict__ wt, const uint64_t *__restrict__ xin, int iters) {
  uint64_t x[WORDS], acc[LINEAR_TJ], sum = 0;
#pragma unroll
  for (int k = 0; k < WORDS; k++) x[k] = xin[(size_t)threadIdx.x * WORDS + k];
#pragma unroll
  for (int t = 0; t < LINEAR_TJ; t++) acc[t] = 0;
  for (int it = 0; it < iters; it++) {
    const int64_t *__restrict__ w = wt + (size_t)(it % STEPS) * WORDS * LINEAR_TJ;   // wave-uniform: scalar loads
#pragma unroll
    for (int k = 0; k < WORDS; k++) {
      if constexpr (NARROW) sum += x[k];
#pragma unroll
      for (int t = 0; t < LINEAR_TJ; t++) acc[t] = linear_mac<NARROW>(acc[t], x[k], NARROW ? w[k * LINEAR_TJ + t] ^ LINEAR_NARROW_BIAS : w[k * LINEAR_TJ + t]);
    }
  }
  uint64_t s = 0;
#pragma unroll
  for (int t = 0; t < LINEAR_TJ; t++) s += NARROW ? acc[t] - (sum << 31) : acc[t];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <bool NARROW>
static void run(const char *name, uint64_t *d_out, const int64_t *d_wt, const uint64_t *d_x, int blocks, int iters) {
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<float> ms;
  for (int r = 0; r < 8; r++) {   // the first one is the warm-up
    CHECK(hipEventRecord(e0, nullptr));
    hipLaunchKernelGGL(mac_kernel<NARROW>, dim3(blocks), dim3(256), 0, nullptr, d_out, d_wt, d_x, iters);
    CHECK(hipEventRecord(e1, nullptr));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipGetLastError());
    float t;
    CHECK(hipEventElapsedTime(&t, e0, e1));
    if (r) ms.push_back(t);
  }
  std::sort(ms.begin(), ms.end());
  const double products = (double)blocks * 256 * iters * WORDS * LINEAR_TJ, med = ms[ms.size() / 2];
  printf("ubench %-6s multiply sequence alone: %d workgroups x 256 lanes x %d steps x %d words x %d rows: median %.4f ms  min %.4f  max %.4f  (7 repeats); %.0f G multiplies/s\n", name,
         blocks, iters, WORDS, LINEAR_TJ, med, ms.front(), ms.back(), products / med / 1e6);
}

int main() {
  int cus = 0;
  CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  const int blocks = cus * 8, iters = 512;   // 8 wavefronts per SIMD asked for, as many as the registers allow resident
  std::vector<int64_t> wt((size_t)STEPS * WORDS * LINEAR_TJ);
  std::vector<uint64_t> x((size_t)256 * WORDS);
  uint64_t s = 0x9E3779B97F4A7C15ULL;
  auto next = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return s ^ (s >> 29); };
  for (auto &v : x) v = next();
  uint64_t *d_out, *d_x;
  int64_t *d_wt;
  CHECK(hipMalloc((void **)&d_out, (size_t)blocks * 256 * 8));
  CHECK(hipMalloc((void **)&d_x, x.size() * 8));
  CHECK(hipMalloc((void **)&d_wt, wt.size() * 8));
  CHECK(hipMemcpy(d_x, x.data(), x.size() * 8, hipMemcpyHostToDevice));
  for (auto &v : wt) v = (int64_t)(int32_t)next();
  CHECK(hipMemcpy(d_wt, wt.data(), wt.size() * 8, hipMemcpyHostToDevice));
  run<true>("narrow", d_out, d_wt, d_x, blocks, iters);
  for (auto &v : wt) v = (int64_t)next();
  CHECK(hipMemcpy(d_wt, wt.data(), wt.size() * 8, hipMemcpyHostToDevice));
  run<false>("wide", d_out, d_wt, d_x, blocks, iters);
  return 0;
}
