// What does the fp64 VALU of one gfx950 SIMD sustain?  CH independent fma chains per wave, W waves per SIMD.
// Reports cycles per wave-instruction seen by one SIMD (4.0 = the 16-lane SIMD saturated by wave64 fp64 ops).
// Also times, the same way (independent chains, 1-4 waves per SIMD), the other instructions the fp64 marching kernel's loop issues
// besides fma / mul / add: v_rcp_f64, v_mov_b64 and v_cndmask_b32 -- does a reciprocal cost one issue slot or several, and do the
// window moves and selects cost what an fma costs?  (bench.py's issue floor counts them all alike.)
// Build: hipcc --offload-arch=gfx950 -O3 -o valu_probe valu_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
template <int CH, int OP>
__global__ __launch_bounds__(256) void k(double *out, double a, double b, int iters) {
    double x[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) x[c] = threadIdx.x * 1e-3 + c;
    const unsigned long long sel = __ballot(threadIdx.x & 1);
    (void)sel;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                if (OP == 0) x[c] = __builtin_fma(x[c], a, b);
                else if (OP == 1) x[c] = x[c] * a;
                else if (OP == 2) x[c] = x[c] + b;
                else if (OP == 3) { float y = (float)x[c]; y = __builtin_fmaf(y, (float)a, (float)b); x[c] = y; }
                else if (OP == 4) x[c] = __builtin_amdgcn_rcp(x[c]);                                   // v_rcp_f64 (x <-> 1/x)
                else if (OP == 5) asm volatile("v_mov_b64 %0, %1" : "=v"(x[c]) : "v"(x[c]));            // (kept by the asm: the compiler would fold it)
                else {   // v_cndmask_b32 on the low word, lanes alternating
                    unsigned lo = (unsigned)__double_as_longlong(x[c]), hi = (unsigned)(__double_as_longlong(x[c]) >> 32);
                    asm volatile("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(lo) : "v"(lo), "v"(hi), "s"(sel));
                    x[c] = __longlong_as_double(((long long)hi << 32) | lo);
                }
            }
    }
    double s = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) s += x[c];
    if (s == 12345.678) out[0] = s;
}
template <int CH, int OP> void run(const char *name, double *out) {
    for (int W = 1; W <= 4; ++W) {
        const int iters = 2000, blocks = 256 * W;
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        hipLaunchKernelGGL((k<CH, OP>), dim3(blocks), dim3(256), 0, 0, out, 1.0000001, 1e-9, iters);
        hipEventRecord(e0);
        hipLaunchKernelGGL((k<CH, OP>), dim3(blocks), dim3(256), 0, 0, out, 1.0000001, 1e-9, iters);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        const double instr_per_simd = (double)iters * 8 * CH * W;     // wave-instructions one SIMD executes
        printf("%-8s chains=%d waves/SIMD=%d : %.3f ms  -> %.2f ns per wave-instr per SIMD (x2.4 GHz = %.2f cycles)\n", name, CH, W, ms,
               ms * 1e6 / instr_per_simd, ms * 1e6 / instr_per_simd * 2.4);
    }
}
int main() {
    double *out; hipMalloc(&out, 8);
    run<1, 0>("fma64", out); run<2, 0>("fma64", out); run<4, 0>("fma64", out); run<8, 0>("fma64", out);
    run<1, 1>("mul64", out); run<4, 1>("mul64", out);
    run<1, 2>("add64", out); run<4, 2>("add64", out);
    run<1, 4>("rcp64", out); run<4, 4>("rcp64", out); run<8, 4>("rcp64", out);
    run<4, 5>("mov64", out); run<8, 5>("mov64", out);
    run<4, 6>("cndmask", out); run<8, 6>("cndmask", out);
    return 0;
}
