// Gradient accumulation over a window of micro-batches (include/fpd_amd.h, fpd_grad_accum_t): one streaming launch over two
// flat fp32 arenas, `grad` and `acc`, in one of three modes -- FIRST acc = grad, ADD acc = acc + grad, FIN grad = acc * s with
// s read from a device float.  The arithmetic is csrc/grad_accum_math.h, which a host build checks against numpy
// (tests/test_accum_cpu.py).  8 (FIRST, FIN) or 12 (ADD) bytes move per element: no LDS, no atomics, one writer per element.
#include "common.h"
#include "conv_dispatch.h"
#include "grad_accum_math.h"

namespace {

// `in` is the arena the mode only reads and `out` the one it writes: (grad, acc) in FIRST and ADD, (acc, grad) in FIN.
template <int MODE>
__global__ __launch_bounds__(256) void grad_accum_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n, int64_t nvec,
                                                         const float* __restrict__ scale_dev) {
    const float s = MODE == FPD_ACCUM_FIN ? *scale_dev : 0.0f;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const float4* i4 = reinterpret_cast<const float4*>(in);
    float4* o4 = reinterpret_cast<float4*>(out);
    for (int64_t i = tid; i < nvec; i += nthr) {
        const float4 x = i4[i];
        float4 y;
        if (MODE == FPD_ACCUM_FIRST) {
            y = x;
        } else if (MODE == FPD_ACCUM_ADD) {
            y = o4[i];
            y.x = fpd_accum_add(y.x, x.x); y.y = fpd_accum_add(y.y, x.y);
            y.z = fpd_accum_add(y.z, x.z); y.w = fpd_accum_add(y.w, x.w);
        } else {
            y.x = fpd_accum_fin(x.x, s); y.y = fpd_accum_fin(x.y, s);
            y.z = fpd_accum_fin(x.z, s); y.w = fpd_accum_fin(x.w, s);
        }
        o4[i] = y;
    }
    for (int64_t i = 4 * nvec + tid; i < n; i += nthr) {
        if (MODE == FPD_ACCUM_FIRST) out[i] = fpd_accum_first(in[i]);
        else if (MODE == FPD_ACCUM_ADD) out[i] = fpd_accum_add(out[i], in[i]);
        else out[i] = fpd_accum_fin(in[i], s);
    }
}

struct byte_range { uintptr_t lo, hi; const char* name; };
inline bool overlap(const byte_range& p, const byte_range& q) { return p.lo < q.hi && q.lo < p.hi; }

}  // namespace

// Validation and the launch's geometry: fpd_grad_accum_launch() below and the query fpd_grad_accum_geometry() both come
// through here.  Pure host code: counts and addresses are looked at, nothing is dereferenced.
int fpd_grad_accum_geometry_of(const fpd_grad_accum_t& a, int* blocks, int64_t* nvec) {
    FPD_REQUIRE(a.mode == FPD_ACCUM_FIRST || a.mode == FPD_ACCUM_ADD || a.mode == FPD_ACCUM_FIN,
                "grad_accum: unknown mode %d (FIRST 0, ADD 1, FIN 2)", a.mode);
    FPD_REQUIRE(a.n >= 0, "grad_accum: n = %lld is negative", (long long)a.n);
    FPD_REQUIRE(a.n < ((int64_t)1 << 60), "grad_accum: n = %lld is too large", (long long)a.n);
    FPD_REQUIRE(a.n == 0 || (a.grad != nullptr && a.acc != nullptr), "grad_accum: null grad or acc with n = %lld", (long long)a.n);
    FPD_REQUIRE(a.mode != FPD_ACCUM_FIN || a.scale_dev != nullptr, "grad_accum: null scale_dev in mode FIN");
    FPD_REQUIRE((((uintptr_t)a.grad | (uintptr_t)a.acc | (uintptr_t)a.scale_dev) & 3) == 0,
                "grad_accum: grad, acc or scale_dev is misaligned (4 bytes)");
    byte_range r[3];
    int nr = 0;
    if (a.n > 0) {
        r[nr++] = {(uintptr_t)a.grad, (uintptr_t)a.grad + 4 * (uintptr_t)a.n, "grad"};
        r[nr++] = {(uintptr_t)a.acc, (uintptr_t)a.acc + 4 * (uintptr_t)a.n, "acc"};
    }
    if (a.scale_dev != nullptr) r[nr++] = {(uintptr_t)a.scale_dev, (uintptr_t)a.scale_dev + 4, "scale_dev"};
    for (int i = 0; i < nr; ++i)
        for (int j = i + 1; j < nr; ++j)
            FPD_REQUIRE(!overlap(r[i], r[j]), "grad_accum: %s overlaps %s", r[i].name, r[j].name);
    const bool aligned = (((uintptr_t)a.grad | (uintptr_t)a.acc) & 15) == 0;
    *nvec = aligned ? a.n / 4 : 0;
    const int64_t rest = a.n - 4 * *nvec;
    *blocks = grid_for(*nvec > rest ? *nvec : rest);
    return 0;
}

int fpd_grad_accum_launch(const fpd_grad_accum_t& a, hipStream_t st) {
    int blocks = 0;
    int64_t nvec = 0;
    const int rc = fpd_grad_accum_geometry_of(a, &blocks, &nvec);
    if (rc) return rc;
    if (a.mode == FPD_ACCUM_FIRST)
        FPD_LAUNCH(grad_accum_kernel<FPD_ACCUM_FIRST>, dim3(blocks), dim3(256), 0, st, (const float*)a.grad, a.acc, a.n, nvec, a.scale_dev);
    else if (a.mode == FPD_ACCUM_ADD)
        FPD_LAUNCH(grad_accum_kernel<FPD_ACCUM_ADD>, dim3(blocks), dim3(256), 0, st, (const float*)a.grad, a.acc, a.n, nvec, a.scale_dev);
    else
        FPD_LAUNCH(grad_accum_kernel<FPD_ACCUM_FIN>, dim3(blocks), dim3(256), 0, st, (const float*)a.acc, a.grad, a.n, nvec, a.scale_dev);
    return 0;
}
