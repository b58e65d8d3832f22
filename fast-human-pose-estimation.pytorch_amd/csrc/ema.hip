// Exponential moving average of a model's flat arenas (include/fpd_amd.h, fpd_ema_t): one streaming launch over all
// segments + a one-thread tick of the update counter.  The arithmetic is csrc/ema_math.h, which a host build checks against
// numpy (tests/test_ema_cpu.py).  12 bytes move per element (source and average read, average written): no LDS, no atomics.
#include "common.h"
#include "conv_dispatch.h"
#include "ema_math.h"

namespace {

struct ema_vecs { int64_t nvec[FPD_EMA_MAX_SEG]; };      // 16-byte vectors of each segment (0: element by element)

// Every thread forms the weight itself from the counter: one float64 division, and no block can see the counter move
// (the tick is a launch of its own behind this one).
__global__ __launch_bounds__(256) void ema_kernel(const fpd_ema_t a, const ema_vecs v) {
    const float w = fpd_ema_weight(*a.updates_dev, a.decay, a.warmup);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
#pragma unroll
    for (int s = 0; s < FPD_EMA_MAX_SEG; ++s) {
        if (s >= a.nseg) break;
        const float* src = a.seg[s].src;
        float* dst = a.seg[s].dst;
        const int64_t n = a.seg[s].n, nvec = v.nvec[s];
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int64_t i = tid; i < nvec; i += nthr) {
            const float4 x = s4[i];
            float4 e = d4[i];
            e.x = fpd_ema_update(e.x, x.x, w); e.y = fpd_ema_update(e.y, x.y, w);
            e.z = fpd_ema_update(e.z, x.z, w); e.w = fpd_ema_update(e.w, x.w, w);
            d4[i] = e;
        }
        for (int64_t i = 4 * nvec + tid; i < n; i += nthr) dst[i] = fpd_ema_update(dst[i], src[i], w);
    }
    for (int64_t i = tid; i < a.copy_n; i += nthr) a.copy_dst[i] = a.copy_src[i];
}
__global__ void ema_tick_kernel(int64_t* updates) { *updates += 1; }

struct byte_range { uintptr_t lo, hi; bool written; };
inline bool overlap(const byte_range& p, const byte_range& q) { return p.lo < q.hi && q.lo < p.hi; }

}  // namespace

// Validation and the launch's geometry: the launch below and the query fpd_ema_geometry() both come through here.
int fpd_ema_geometry_of(const fpd_ema_t& a, int* blocks, int64_t* nvec) {
    FPD_REQUIRE(a.nseg >= 1 && a.nseg <= FPD_EMA_MAX_SEG, "ema: nseg = %d outside 1..%d", a.nseg, FPD_EMA_MAX_SEG);
    FPD_REQUIRE(a.updates_dev != nullptr, "ema: null update counter (updates_dev)");
    FPD_REQUIRE(a.decay >= 0.0 && a.decay < 1.0, "ema: decay %g outside [0, 1)", a.decay);
    FPD_REQUIRE(a.copy_n >= 0, "ema: copy_n = %lld is negative", (long long)a.copy_n);
    FPD_REQUIRE(a.copy_n == 0 || (a.copy_src != nullptr && a.copy_dst != nullptr), "ema: null pointer with copy_n = %lld", (long long)a.copy_n);
    byte_range r[2 * FPD_EMA_MAX_SEG + 3];
    int nr = 0;
    int64_t work = a.copy_n;
    for (int s = 0; s < a.nseg; ++s) {
        const fpd_ema_seg_t& g = a.seg[s];
        FPD_REQUIRE(g.n >= 0, "ema: segment %d has a negative n = %lld", s, (long long)g.n);
        FPD_REQUIRE(g.n < ((int64_t)1 << 60), "ema: segment %d: n = %lld is too large", s, (long long)g.n);
        FPD_REQUIRE(g.n == 0 || (g.src != nullptr && g.dst != nullptr), "ema: segment %d: null pointer with n = %lld", s, (long long)g.n);
        const bool aligned = (((uintptr_t)g.src | (uintptr_t)g.dst) & 15) == 0;
        nvec[s] = aligned ? g.n / 4 : 0;
        const int64_t rest = g.n - 4 * nvec[s];
        work = work > nvec[s] ? work : nvec[s];
        work = work > rest ? work : rest;
        if (g.n > 0) {
            r[nr++] = {(uintptr_t)g.src, (uintptr_t)g.src + 4 * (uintptr_t)g.n, false};
            r[nr++] = {(uintptr_t)g.dst, (uintptr_t)g.dst + 4 * (uintptr_t)g.n, true};
        }
    }
    if (a.copy_n > 0) {
        r[nr++] = {(uintptr_t)a.copy_src, (uintptr_t)a.copy_src + 8 * (uintptr_t)a.copy_n, false};
        r[nr++] = {(uintptr_t)a.copy_dst, (uintptr_t)a.copy_dst + 8 * (uintptr_t)a.copy_n, true};
    }
    r[nr++] = {(uintptr_t)a.updates_dev, (uintptr_t)a.updates_dev + 8, true};
    for (int i = 0; i < nr; ++i)
        for (int j = i + 1; j < nr; ++j)
            FPD_REQUIRE(!((r[i].written || r[j].written) && overlap(r[i], r[j])),
                        "ema: a written range overlaps another range (the average must not alias its source, another segment or the counter)");
    *blocks = grid_for(work);
    return 0;
}

int fpd_ema_launch(const fpd_ema_t& a, hipStream_t st) {
    ema_vecs v = {};
    int blocks = 0;
    const int rc = fpd_ema_geometry_of(a, &blocks, v.nvec);
    if (rc) return rc;
    FPD_LAUNCH(ema_kernel, dim3(blocks), dim3(256), 0, st, a, v);
    FPD_LAUNCH(ema_tick_kernel, dim3(1), dim3(1), 0, st, a.updates_dev);
    return 0;
}
