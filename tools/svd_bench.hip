// Micro-benchmark of the PBD tetrahedral projection (pbd_project.h tet_core) - development aid, not part of the product.
// Three forms: VARIANT 0 = tet_core (closed-form start, round 6), VARIANT 2 = the plain one-sided Jacobi iteration from
// V = I (rounds 1-5), VARIANT 3 = tet_rows.h (VARIANT 0's arithmetic on row pairs, rare paths behind uniform tests: k_layer's form).
// Two element classes:
//   healthy    a sheared, stretched element (what a perturbed rest state looks like: the plain iteration takes 3-4 sweeps)
//   flattened  all four nodes in the plane y = const (BASELINE config 2 after its first tick: every element lies on the floor,
//              one column of F is exactly zero)
// One workgroup per compute unit runs STEPS dependent projections per lane, 1 to 4 wavefronts per SIMD: one wavefront per SIMD is
// k_layer's situation at 100k particles (a colour step lasts as long as one wavefront's instruction stream), four per SIMD is
// the throughput limit (time / 4 = the issue time of the stream).
//
// Last, the issue cost of packed fp32 for a wavefront alone on its SIMD: a stream of independent v_pk_fma_f32 on aligned pairs
// against twice as many v_fma_f32 (build this file with -fno-slp-vectorize as well: the scalar stream then stays scalar, and the
// projection figures are those of the scalar build).  The scalar stream runs twice more: with lanes 0-31 alone active (does a
// half-empty wavefront issue faster?) and with two wavefronts per SIMD (what a second wavefront's instruction costs the first) -
// the two numbers that price any form of the projection that splits an element over lanes or wavefronts.
//
// build: hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -I pies_amd/csrc -I include tools/svd_bench.hip -o /tmp/svd_bench
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "pbd_project.h"
#include "tet_rows.h"

using namespace pies;

template <int VARIANT, bool FLAT> __global__ void k_chain(float4* out, int steps) {
  const int t = threadIdx.x + blockIdx.x * blockDim.x;
  const float e = 0.001f * static_cast<float>(t % 97);
  const float y0 = FLAT ? 0.475f : 0.02f;
  float4 x1 = make_float4(0.01f + e, y0, -0.01f, 1.f), x2 = make_float4(1.1f + e, FLAT ? y0 : 0.05f, 0.02f, 1.f);
  float4 x3 = make_float4(-0.03f, FLAT ? y0 : 0.93f + e, 0.04f, 1.f), x4 = make_float4(0.02f, FLAT ? y0 : -0.04f, 1.07f - e, 1.f);
  const float4 a0 = make_float4(1.f, 0.f, 0.f, 0.f), a1 = make_float4(1.f, 0.f, 0.f, 0.f), a2 = make_float4(1.f, 0.8f, 1.0f, 0.05f);
  for (int s = 0; s < steps; ++s) {
    if (VARIANT == 3) rows::tet_rows(x1, x2, x3, x4, rows::rest_of(a0, a1, a2));
    else tet_core<VARIANT == 3 ? 0 : VARIANT>(x1, x2, x3, x4, a0, a1, a2);
    // keep the element from collapsing towards the origin (quirk Q2) so that every step does a full decomposition
    x2.x += 1.0f; x4.z += 1.0f;
    x4.x -= 0.27f; x2.z -= 0.19f;
    if (FLAT) { x1.y = y0; x2.y = y0; x3.y = y0; x4.y = y0; x3.x += 0.4f; x3.z += 0.6f; }  // (the floor clamp)
    else { x3.y += 1.0f; x2.y += 0.31f; x3.z += 0.23f; }
  }
  out[t] = make_float4(x1.x + x2.x, x1.y + x3.y, x1.z + x4.z, x2.y + x3.z + x4.x);
}

template <int VARIANT, bool FLAT> static void run(const char* name, float4* d) {
  const int cus = 256, steps = 200;
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  std::printf("%s\n", name);
  for (int waves = 1; waves <= 4; ++waves) {
    const int threads = 256 * waves;
    hipLaunchKernelGGL((k_chain<VARIANT, FLAT>), dim3(cus), dim3(threads), 0, 0, d, steps);  // warm
    hipDeviceSynchronize();
    float best = 1e30f;
    for (int rep = 0; rep < 5; ++rep) {
      hipEventRecord(e0, 0);
      hipLaunchKernelGGL((k_chain<VARIANT, FLAT>), dim3(cus), dim3(threads), 0, 0, d, steps);
      hipEventRecord(e1, 0);
      hipEventSynchronize(e1);
      float ms = 0.f;
      hipEventElapsedTime(&ms, e0, e1);
      best = ms < best ? ms : best;
    }
    std::vector<float4> h(4);
    hipMemcpy(h.data(), d, sizeof(float4) * 4, hipMemcpyDeviceToHost);
    std::printf("  %d wavefront(s) per SIMD: %.3f us per projection step  (checksum %.6f)\n", waves, 1e3 * best / steps,
                h[0].x + h[1].y + h[2].z + h[3].w);
  }
}

// 16 independent accumulators per lane: 8 packed fused multiply-adds, or 16 scalar ones, per round
typedef float pk2 __attribute__((ext_vector_type(2)));
// HALF: lanes 32-63 of every wavefront leave at once
template <bool PACKED, bool HALF = false> __global__ void k_issue(float4* out, int rounds, float m0, float c0) {  // (m0, c0 from the host: operands in registers)
  const float t = 1.0f + 1.0e-6f * static_cast<float>(threadIdx.x);
  if (HALF && (threadIdx.x & 63u) >= 32u) return;
  if (PACKED) {
    pk2 a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = pk2{t + static_cast<float>(i), t - static_cast<float>(i)};
    const pk2 m = {m0, m0 + 0.002f}, c = {c0, -c0};
    for (int r = 0; r < rounds; ++r)
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = __builtin_elementwise_fma(a[i], m, c);
    pk2 s = a[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s += a[i];
    out[threadIdx.x + blockIdx.x * blockDim.x] = make_float4(s.x, s.y, 0.f, 0.f);
  } else {
    float a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = t + static_cast<float>(i);
    const float m = m0, c = c0;
    for (int r = 0; r < rounds; ++r)
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = fmaf(a[i], m, c);
    float s = a[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) s += a[i];
    out[threadIdx.x + blockIdx.x * blockDim.x] = make_float4(s, 0.f, 0.f, 0.f);
  }
}
template <bool PACKED, bool HALF = false> static float issue_ns(float4* d, int threads = 256) {  // ns per instruction of one wavefront; 256 threads: one wavefront per SIMD
  const int rounds = 2000, per_round = PACKED ? 64 : 128;
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipLaunchKernelGGL((k_issue<PACKED, HALF>), dim3(256), dim3(threads), 0, 0, d, rounds, 0.999f, 1.0e-3f);
  hipDeviceSynchronize();
  float best = 1e30f;
  for (int rep = 0; rep < 5; ++rep) {
    hipEventRecord(e0, 0);
    hipLaunchKernelGGL((k_issue<PACKED, HALF>), dim3(256), dim3(threads), 0, 0, d, rounds, 0.999f, 1.0e-3f);
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    best = ms < best ? ms : best;
  }
  return 1.0e6f * best / (static_cast<float>(rounds) * per_round);
}

int main() {
  float4* d;
  hipMalloc(&d, sizeof(float4) * 256 * 1024);
  {
    const float pk = issue_ns<true>(d), sc = issue_ns<false>(d);
    std::printf("issue cost, one wavefront per SIMD, independent instructions: v_pk_fma_f32 %.3f ns, v_fma_f32 %.3f ns: a packed one costs %.2f scalar ones\n",
                pk, sc, pk / sc);
    // cycles at the clock the device reports (hipDeviceAttributeClockRate, kHz): per instruction of ONE wavefront's stream
    int khz = 0;
    hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0);
    const float half = issue_ns<false, true>(d), two = issue_ns<false>(d, 512);
    const float cyc = 1.0e-6f * static_cast<float>(khz);
    std::printf("independent v_fma_f32 per wavefront, at %d MHz: one wavefront per SIMD %.3f ns = %.2f cycles; lanes 0-31 alone %.3f ns = %.2f cycles; "
                "two wavefronts per SIMD %.3f ns = %.2f cycles each (%.2f per SIMD)\n", khz / 1000, sc, sc * cyc, half, half * cyc, two, two * cyc, 0.5f * two * cyc);
  }
  run<3, false>("healthy element, tet_rows.h (row pairs)", d);
  run<3, true>("flattened element (y = const), tet_rows.h (row pairs)", d);
  run<2, false>("healthy element, plain Jacobi iteration from V = I (rounds 1-5)", d);
  run<0, false>("healthy element, closed-form start (round 6)", d);
  run<2, true>("flattened element (y = const), plain Jacobi iteration", d);
  run<0, true>("flattened element (y = const), closed-form start's direct path", d);
  return 0;
}
