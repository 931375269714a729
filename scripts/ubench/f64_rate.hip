// Issue rate of the binary64 VALU instructions k_scene_interpolants (raster_attr.hip, docs/DESIGN_DETAILS.md §7.18) is made of on gfx950: v_add_f64, v_mul_f64,
// v_fma_f64 (for comparison: the contract uses no fused operation), v_cvt_f64_f32 / v_cvt_f32_f64 and the IEEE quotient as the compiler expands it. 8 independent
// chains per lane, 2048 workgroups of 256 lanes (8 waves per SIMD), 40 launches after a spin-up. Prints G lane-operations/s. usage: ./f64_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define CHAINS(OP) for (int i = 0; i < iters; ++i) { OP(x0) OP(x1) OP(x2) OP(x3) OP(x4) OP(x5) OP(x6) OP(x7) }
#define DECL double x0 = 1.0 + threadIdx.x * 1e-3, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7; double h = w + threadIdx.x * 1e-9;
#define FIN out[blockIdx.x * blockDim.x + threadIdx.x] = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
__global__ void k_add(double* out, double w, int iters) { DECL
#define OPA(x) asm volatile("v_add_f64 %0, %0, %1" : "+v"(x) : "v"(h));
    CHAINS(OPA) FIN }
__global__ void k_mul(double* out, double w, int iters) { DECL
#define OPM(x) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(x) : "v"(h));
    CHAINS(OPM) FIN }
__global__ void k_fma(double* out, double w, int iters) { DECL
#define OPF(x) asm volatile("v_fma_f64 %0, %0, %1, %1" : "+v"(x) : "v"(h));
    CHAINS(OPF) FIN }
__global__ void k_cvt(double* out, double w, int iters) { DECL float t;      // one widening and one narrowing conversion per step: counted as two operations
#define OPC(x) asm volatile("v_cvt_f32_f64 %1, %0\n\tv_cvt_f64_f32 %0, %1" : "+v"(x), "=&v"(t));
    CHAINS(OPC) FIN }
__global__ void k_div(double* out, double w, int iters) { DECL              // x = h / x: the correctly rounded quotient, as hipcc expands it
#define OPD(x) x = h / x; asm volatile("" : "+v"(x));
    CHAINS(OPD) FIN }

template <class K> static double rate(K kernel, double* out, int iters, double opsPerStep) {
    const int blocks = 2048, lanes = 256, launches = 40;
    hipEvent_t a, b; (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    for (int i = 0; i < 5; ++i) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(lanes), 0, 0, out, 1.0000001, iters);
    (void)hipEventRecord(a, 0);
    for (int i = 0; i < launches; ++i) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(lanes), 0, 0, out, 1.0000001, iters);
    (void)hipEventRecord(b, 0);
    if (hipEventSynchronize(b) != hipSuccess) { fprintf(stderr, "kernel failed\n"); exit(1); }
    float ms = 0; (void)hipEventElapsedTime(&ms, a, b);
    return (double)blocks * lanes * launches * iters * 8.0 * opsPerStep / (ms * 1e-3) / 1e9;
}

int main() {
    double* out = nullptr;
    if (hipMalloc(&out, 2048 * 256 * sizeof(double)) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    printf("{\"bench\": \"f64_rate\", \"unit\": \"G lane-operations/s\", \"v_add_f64\": %.1f, \"v_mul_f64\": %.1f, \"v_fma_f64\": %.1f, \"cvt_f32_f64_pair\": %.1f, \"div_f64\": %.1f}\n",
           rate(k_add, out, 2000, 1), rate(k_mul, out, 2000, 1), rate(k_fma, out, 2000, 1), rate(k_cvt, out, 2000, 2), rate(k_div, out, 200, 1));
    (void)hipFree(out);
    return 0;
}
