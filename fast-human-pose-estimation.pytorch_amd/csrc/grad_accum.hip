// Gradient accumulation over a window of micro-batches (include/fpd_amd.h, fpd_grad_accum_t): one streaming launch over two
// flat fp32 arenas, `grad` and `acc`, in one of three modes -- FIRST acc = grad, ADD acc = acc + grad, FIN grad = acc * s with
// s read from a device float.  The arithmetic is csrc/grad_accum_math.h, which a host build checks against numpy
// (tests/test_accum_cpu.py).  8 (FIRST, FIN) or 12 (ADD) bytes move per element: no LDS, no atomics, one writer per element.
#include "flat_stream.h"
#include "grad_accum_math.h"

namespace {

// `in` is the arena the mode only reads and `out` the one it writes: (grad, acc) in FIRST and ADD, (acc, grad) in FIN.
template <int MODE>
__global__ __launch_bounds__(256) void grad_accum_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n, int64_t nvec,
                                                         const float* __restrict__ scale_dev) {
    const float s = MODE == FPD_ACCUM_FIN ? *scale_dev : 0.0f;
    if constexpr (MODE == FPD_ACCUM_ADD)
        flat_walk(n, nvec, nullptr, [](int64_t, float& y, float x) { y = fpd_accum_add(y, x); }, out, in);
    else
        flat_walk(n, nvec, nullptr, [&](int64_t, float& y, float x) { y = MODE == FPD_ACCUM_FIRST ? fpd_accum_first(x) : fpd_accum_fin(x, s); },
                  flat_out{out}, in);
}

}  // namespace

// Validation and the launch's geometry: fpd_grad_accum_launch() below and the query fpd_grad_accum_geometry() both come
// through here.  Pure host code: counts and addresses are looked at, nothing is dereferenced.
int fpd_grad_accum_geometry_of(const fpd_grad_accum_t& a, int* blocks, int64_t* nvec) {
    FPD_REQUIRE(a.mode == FPD_ACCUM_FIRST || a.mode == FPD_ACCUM_ADD || a.mode == FPD_ACCUM_FIN,
                "grad_accum: unknown mode %d (FIRST 0, ADD 1, FIN 2)", a.mode);
    if (const int rc = require_flat_n("grad_accum", a.n)) return rc;
    FPD_REQUIRE(a.n == 0 || (a.grad != nullptr && a.acc != nullptr), "grad_accum: null grad or acc with n = %lld", (long long)a.n);
    FPD_REQUIRE(a.mode != FPD_ACCUM_FIN || a.scale_dev != nullptr, "grad_accum: null scale_dev in mode FIN");
    FPD_REQUIRE((((uintptr_t)a.grad | (uintptr_t)a.acc | (uintptr_t)a.scale_dev) & 3) == 0,
                "grad_accum: grad, acc or scale_dev is misaligned (4 bytes)");
    byte_range r[3];      // marked written whatever the mode: grad and acc swap roles, and nothing may lie over the scale
    int nr = 0;
    if (a.n > 0) {
        r[nr++] = range_of(a.grad, 4 * (uint64_t)a.n, true, "grad");
        r[nr++] = range_of(a.acc, 4 * (uint64_t)a.n, true, "acc");
    }
    if (a.scale_dev != nullptr) r[nr++] = range_of(a.scale_dev, 4, true, "scale_dev");
    if (const int rc = require_disjoint("grad_accum", r, nr)) return rc;
    flat_geometry(a.n, (uintptr_t)a.grad | (uintptr_t)a.acc, nullptr, nvec, blocks);
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
