// Global gradient-norm clipping of a flat fp32 arena (include/fpd_amd.h, fpd_grad_clip_t): three launches on one stream --
// per-block float64 sums of squares, one block that adds them in index order and forms norm and coefficient
// (csrc/grad_clip_math.h, which a host build checks against numpy, tests/test_clip_cpu.py), and the in-place scale, which
// every thread leaves at once when the coefficient is exactly 1.  No atomics: each partial has one writer and the additions
// run in a fixed order, so the result is a function of the values and the grid, and the grid of n and the base's alignment.
#include "flat_stream.h"
#include "grad_clip_math.h"

namespace {

// Sum over the block's 256 threads, the same on every call: the xor butterfly inside a wave, then the four waves in order.
__device__ __forceinline__ double block_sum_d(double v, double* lds) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// every product is exact in float64 (two 24-bit significands), so whether the compiler fuses it into the addition is moot
__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, int64_t nvec, double* __restrict__ partial) {
    __shared__ double lds[4];
    double acc = 0.0;
    flat_walk(n, nvec, nullptr, [&](int64_t, float x) { acc += sq(x); }, g);      // read only: a thread's squares add up in index order
    const double s = block_sum_d(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_clip_final_kernel(const double* __restrict__ partial, int blocks, float max_norm, float* __restrict__ out,
                                                              int64_t* __restrict__ counters) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) acc += partial[i];
    const double s = block_sum_d(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = fpd_clip_norm(s);
        const float coef = fpd_clip_coef(norm, max_norm);
        out[0] = norm;
        out[1] = coef;
        if (counters != nullptr) {
            counters[0] += 1;
            counters[1] += coef < 1.0f ? 1 : 0;
            counters[2] += isfinite(norm) ? 0 : 1;
        }
    }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(float* __restrict__ g, int64_t n, int64_t nvec, const float* __restrict__ out) {
    const float coef = out[1];
    if (coef == 1.0f) return;                  // not clipped (a NaN coefficient is not 1: it is written into every element)
    flat_walk(n, nvec, nullptr, [&](int64_t, float& x) { x = fpd_clip_scale(x, coef); }, g);
}

}  // namespace

// Bytes of `partial` that serve an arena of n elements at any alignment: one float64 per block of the largest grid.
int64_t fpd_grad_clip_scratch_size(int64_t n) {
    if (const int rc = require_flat_n("grad_clip", n)) return rc;
    return 8 * (int64_t)grid_for(n);
}

// Validation and the launches' geometry: fpd_grad_clip_launch() below and the query fpd_grad_clip_geometry() both come
// through here.  Pure host code: counts and addresses are looked at, nothing is dereferenced.
int fpd_grad_clip_geometry_of(const fpd_grad_clip_t& a, int* blocks, int64_t* nvec) {
    if (const int rc = require_flat_n("grad_clip", a.n)) return rc;
    FPD_REQUIRE(a.n == 0 || a.grad != nullptr, "grad_clip: null grad with n = %lld", (long long)a.n);
    FPD_REQUIRE(a.out != nullptr, "grad_clip: null out");
    FPD_REQUIRE(a.partial != nullptr, "grad_clip: null partial (scratch)");
    FPD_REQUIRE(a.max_norm > 0.0f, "grad_clip: max_norm = %g must be positive (+inf measures without clipping)", (double)a.max_norm);      // refuses a NaN too
    const int64_t need = fpd_grad_clip_scratch_size(a.n);
    FPD_REQUIRE(a.partial_bytes >= need, "grad_clip: scratch of %lld bytes is too small, fpd_grad_clip_scratch_bytes(%lld) = %lld",
                (long long)a.partial_bytes, (long long)a.n, (long long)need);
    FPD_REQUIRE(((uintptr_t)a.partial & 7) == 0, "grad_clip: partial is misaligned (8 bytes)");
    FPD_REQUIRE(((uintptr_t)a.out & 3) == 0 && ((uintptr_t)a.counters & 7) == 0 && ((uintptr_t)a.grad & 3) == 0,
                "grad_clip: grad, out or counters is misaligned (4, 4 and 8 bytes)");
    byte_range r[4];      // all four are written, grad by the scale
    int nr = 0;
    if (a.n > 0) r[nr++] = range_of(a.grad, 4 * (uint64_t)a.n, true, "grad");
    r[nr++] = range_of(a.partial, (uint64_t)a.partial_bytes, true, "partial");
    r[nr++] = range_of(a.out, 8, true, "out");
    if (a.counters != nullptr) r[nr++] = range_of(a.counters, 24, true, "counters");
    if (const int rc = require_disjoint("grad_clip", r, nr)) return rc;
    flat_geometry(a.n, (uintptr_t)a.grad, nullptr, nvec, blocks);
    return 0;
}

int fpd_grad_clip_launch(const fpd_grad_clip_t& a, hipStream_t st) {
    int blocks = 0;
    int64_t nvec = 0;
    const int rc = fpd_grad_clip_geometry_of(a, &blocks, &nvec);
    if (rc) return rc;
    FPD_LAUNCH(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, st, (const float*)a.grad, a.n, nvec, a.partial);
    FPD_LAUNCH(grad_clip_final_kernel, dim3(1), dim3(256), 0, st, (const double*)a.partial, blocks, a.max_norm, a.out, a.counters);
    FPD_LAUNCH(grad_scale_kernel, dim3(blocks), dim3(256), 0, st, a.grad, a.n, nvec, (const float*)a.out);
    return 0;
}
