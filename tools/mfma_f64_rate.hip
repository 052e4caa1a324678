// tools/mfma_f64_rate.hip -- the rate of a bare loop of v_mfma_f64_16x16x4_f64 on this device: what tools/bootstrap_time.py sets beside the float64
// FLOP/s of ca_clone_loglik_reweighted's products.  Every wave issues the instruction back to back into TILES independent accumulators (no memory traffic
// inside the loop); blocks x waves fill every SIMD `waves` deep.  Prints one JSON line.
//   build: hipcc -O3 --offload-arch=gfx950 -o tools/mfma_f64_rate.bin tools/mfma_f64_rate.hip
//   run:   tools/mfma_f64_rate.bin [waves_per_simd = 2] [iterations = 200000]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int TILES = 8;

__global__ void __launch_bounds__(256) k_rate(double* out, int iters, double a0, double b0) {
  f64x4 acc[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc[t] = (f64x4){0.0, 0.0, 0.0, 0.0};
  const double a = a0 + threadIdx.x * 1e-9, b = b0 + blockIdx.x * 1e-9;
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < TILES; ++t) s += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;   // (keeps the loop alive)
}

#define CK(x)                                                                        \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
  } while (0)

int main(int argc, char** argv) {
  const int waves = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 200000;
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, 0));
  const int blocks = p.multiProcessorCount * waves;   // 256 threads = one wave per SIMD of a CU
  double* out = nullptr;
  CK(hipMalloc(&out, (size_t)blocks * 256 * sizeof(double)));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int rep = 0; rep < 6; ++rep) {   // (the first is the warm-up)
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_rate, dim3(blocks), dim3(256), 0, 0, out, iters, 1.0, 0.5);
    CK(hipGetLastError());
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (rep > 0 && ms < best) best = ms;
  }
  const double flop = 2.0 * 16 * 16 * 4 * (double)TILES * iters * (double)blocks * 4;
  printf("{\"mfma_f64_16x16x4_bare_loop_tflops\": %.2f, \"best_ms\": %.3f, \"compute_units\": %d, \"waves_per_simd\": %d, \"iterations\": %d}\n", flop / (best * 1e-3) / 1e12,
         best, p.multiProcessorCount, waves, iters);
  CK(hipFree(out));
  return 0;
}
