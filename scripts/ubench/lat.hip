// micro-benchmarks of the latencies the dense phase of the IPM is built from (gfx950): dependent fp64 FMA / rcp chains, dependent and independent
// v_mfma_f64_16x16x4, MFMA result -> VALU use, LDS write -> read round trip, s_barrier with 8 waves; the scalar load of a cached line as an out-of-line
// function looked up its LDS base (kernel ks).  One workgroup; prints cycles (s_memtime).
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double v4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(512) void k(double* out, long long* t, int reps) {
    __shared__ double lds[2048];
    const int tid = threadIdx.x;
    double x = 1.0 + tid * 1e-9, y = 0.999;
    long long t0, t1;
    // 1. dependent FMA chain
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) { x = fma(x, y, 1e-9); x = fma(x, y, 1e-9); x = fma(x, y, 1e-9); x = fma(x, y, 1e-9); }
    asm volatile("" : "+v"(x)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[0] = (t1 - t0);
    // 2. dependent rcp chain
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) { x = __builtin_amdgcn_rcp(x); x = __builtin_amdgcn_rcp(x); x = __builtin_amdgcn_rcp(x); x = __builtin_amdgcn_rcp(x); }
    asm volatile("" : "+v"(x)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[1] = (t1 - t0);
    // 3. dependent MFMA chain (same accumulator)
    v4 c = {0, 0, 0, 0}, c2 = {0, 0, 0, 0}, c3 = {0, 0, 0, 0}, c4 = {0, 0, 0, 0};
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) { c = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0); c = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0);
                                     c = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0); c = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0); }
    asm volatile("" : "+v"(c)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[2] = (t1 - t0);
    // 4. independent MFMAs (4 accumulators), all 8 waves
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) { c = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0); c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c2, 0, 0, 0);
                                     c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c3, 0, 0, 0); c4 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c4, 0, 0, 0); }
    asm volatile("" : "+v"(c), "+v"(c2), "+v"(c3), "+v"(c4)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[3] = (t1 - t0);
    // 5. one MFMA then use of its result by the VALU (latency issue -> readable), wave 0 only measured but all waves run
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) { c = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0); x = fma(c[0], 1e-300, x); x = fma(x, y, 1e-9); x = fma(x, y, 1e-9); x = fma(x, y, 1e-9); }
    asm volatile("" : "+v"(x)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[4] = (t1 - t0);
    // 6. LDS write -> read round trip (same wave)
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) { lds[tid] = x; x = lds[(tid + 1) & 511 & ~63 | (tid & 63)]; lds[tid + 512] = x; x = lds[512 + tid]; lds[tid + 1024] = x; x = lds[1024 + tid]; lds[tid + 1536] = x; x = lds[1536 + tid]; }
    asm volatile("" : "+v"(x)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[5] = (t1 - t0);
    // 7. barriers
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) { __syncthreads(); __syncthreads(); __syncthreads(); __syncthreads(); }
    t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[6] = (t1 - t0);
    // 8. only wave 0 issues MFMAs (others idle at the barrier): one wave's issue rate on its own
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    if (tid < 64) for (int i = 0; i < reps; i++) { c = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0); c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c2, 0, 0, 0);
                                     c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c3, 0, 0, 0); c4 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c4, 0, 0, 0); }
    asm volatile("" : "+v"(c), "+v"(c2), "+v"(c3), "+v"(c4)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[7] = (t1 - t0);
    // 9. v_cndmask / int op issue: independent 32-bit ops
    int a = tid, b = tid * 3;
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) { a = a * 3 + b; b = b ^ (a >> 3); a = a + (b << 1); b = b + 7 * a; }
    asm volatile("" : "+v"(a), "+v"(b)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[8] = (t1 - t0);
    out[tid] = x + c[0] + c2[1] + c3[2] + c4[3] + a + b;
}
// What the look-up of the dynamic-LDS base cost an out-of-line device function (the compiler's per-kernel table in memory, docs/history.md): chains of
// DEPENDENT s_load_dword of one line that stays in the scalar cache (every entry of `chain` is 0: the next address is the pointer plus what was loaded),
// each followed by the full wait it needs -- lgkmcnt counts LDS and scalar-memory operations together and scalar loads return out of order.
//   0: the load and its wait alone     1: eight ds_read_b64 requested in front of the load: the wait drains them too
//   2: a phase entry: s_getpc_b64, four scalar adds, the load, its wait, then the first LDS read, which needs the loaded base, and its wait
__global__ __launch_bounds__(512) void ks(const unsigned* chain, long long* t, double* out, int reps) {
    __shared__ double lds[1024];
    const int tid = threadIdx.x;
    lds[tid] = 0.0; lds[tid + 512] = 0.0;
    const unsigned la = (unsigned)(size_t)(__attribute__((address_space(3))) double*)lds + 8u * tid;
    unsigned long long p = (unsigned long long)chain;
    unsigned v;
    double acc = 0;
    long long t0, t1;
#define SLOAD "s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)"
    asm volatile(SLOAD : "=s"(v) : "s"(p) : "memory"); p += v;      // (the line is in the cache from here on)
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) {
        #pragma unroll
        for (int r = 0; r < 4; r++) { asm volatile(SLOAD : "=s"(v) : "s"(p) : "memory"); p += v; }
    }
    asm volatile("" : "+s"(p)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[0] = (t1 - t0);
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) {
        #pragma unroll
        for (int r = 0; r < 4; r++) {
            double d0, d1, d2, d3, d4, d5, d6, d7;
            asm volatile("ds_read_b64 %0, %9\n\tds_read_b64 %1, %9 offset:4096\n\tds_read_b64 %2, %9\n\tds_read_b64 %3, %9 offset:4096\n\t"
                         "ds_read_b64 %4, %9\n\tds_read_b64 %5, %9 offset:4096\n\tds_read_b64 %6, %9\n\tds_read_b64 %7, %9 offset:4096\n\t"
                         "s_load_dword %8, %10, 0x0\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3), "=&v"(d4), "=&v"(d5), "=&v"(d6), "=&v"(d7), "=&s"(v) : "v"(la), "s"(p) : "memory");
            p += v; acc += ((d0 + d1) + (d2 + d3)) + ((d4 + d5) + (d6 + d7));
        }
    }
    asm volatile("" : "+s"(p)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[1] = (t1 - t0);
    __syncthreads(); t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; i++) {
        #pragma unroll
        for (int r = 0; r < 4; r++) {
            unsigned long long pc; unsigned a = 0, b = 0, x;
            asm volatile("s_getpc_b64 %1\n\ts_add_u32 %2, %2, 0\n\ts_addc_u32 %3, %3, 0\n\ts_add_u32 %2, %2, 0\n\ts_addc_u32 %3, %3, 0\n\t"
                         "s_load_dword %0, %4, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v), "=&s"(pc), "+s"(a), "+s"(b) : "s"(p) : "memory", "scc");
            const unsigned addr = la + v;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(x) : "v"(addr) : "memory");
            p += (unsigned)__builtin_amdgcn_readfirstlane((int)x) + (a & b);
        }
    }
    asm volatile("" : "+s"(p)); t1 = __builtin_amdgcn_s_memtime(); if (tid == 0) t[2] = (t1 - t0);
    out[tid] = acc + (double)(p - (unsigned long long)chain);
}
int main() {
    double* out; long long* t; hipMalloc(&out, 512 * 8); hipMalloc(&t, 16 * 8);
    const int reps = 256;
    for (int it = 0; it < 2; it++) hipLaunchKernelGGL(k, dim3(1), dim3(512), 0, 0, out, t, reps);
    long long h[16]; hipMemcpy(h, t, 16 * 8, hipMemcpyDeviceToHost);
    const char* names[] = {"dependent fma f64", "dependent rcp f64", "dependent mfma f64 16x16x4 (same acc), 8 waves", "independent mfma x4, 8 waves", "mfma -> valu use + 3 fma", "lds write->read round trip", "s_barrier (8 waves)", "independent mfma x4, ONE wave", "dependent int ops"};
    for (int i = 0; i < 9; i++) printf("%-55s %8.1f cycles per op\n", names[i], (double)h[i] / (reps * 4));
    unsigned* chain; hipMalloc(&chain, 256); hipMemset(chain, 0, 256);
    for (int it = 0; it < 2; it++) hipLaunchKernelGGL(ks, dim3(1), dim3(512), 0, 0, chain, t, out, reps);
    if (hipMemcpy(h, t, 16 * 8, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    const char* snames[] = {"dependent s_load_dword of a cached line + lgkmcnt(0)", "... with eight ds_read_b64 in flight before the wait",
                            "phase entry: getpc, 4 scalar adds, s_load, wait, ds_read, wait"};
    for (int i = 0; i < 3; i++) printf("%-62s %8.1f cycles per op\n", snames[i], (double)h[i] / (reps * 4));
    return 0;
}
