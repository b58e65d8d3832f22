// Exponential moving average of a model's flat arenas (include/fpd_amd.h, fpd_ema_t): one streaming launch over all
// segments + a one-thread tick of the update counter.  The arithmetic is csrc/ema_math.h, which a host build checks against
// numpy (tests/test_ema_cpu.py).  12 bytes move per element (source and average read, average written): no LDS, no atomics.
#include "flat_stream.h"
#include "ema_math.h"

namespace {

struct ema_vecs { int64_t nvec[FPD_EMA_MAX_SEG]; };      // 16-byte vectors of each segment (0: element by element)

// Every thread forms the weight itself from the counter: one float64 division, and no block can see the counter move
// (the tick is a launch of its own behind this one).
__global__ __launch_bounds__(256) void ema_kernel(const fpd_ema_t a, const ema_vecs v) {
    const float w = fpd_ema_weight(*a.updates_dev, a.decay, a.warmup);
#pragma unroll
    for (int s = 0; s < FPD_EMA_MAX_SEG; ++s) {
        if (s >= a.nseg) break;
        flat_walk(a.seg[s].n, v.nvec[s], nullptr, [&](int64_t, float& e, float x) { e = fpd_ema_update(e, x, w); },
                  a.seg[s].dst, (const float*)a.seg[s].src);
    }
    for (int64_t i = flat_tid(); i < a.copy_n; i += flat_nthr()) a.copy_dst[i] = a.copy_src[i];
}

// what the messages call a segment, its source and its average
const char* const seg_names[FPD_EMA_MAX_SEG][3] = {{"ema: segment 0", "seg[0].src", "seg[0].dst"}, {"ema: segment 1", "seg[1].src", "seg[1].dst"},
                                                   {"ema: segment 2", "seg[2].src", "seg[2].dst"}, {"ema: segment 3", "seg[3].src", "seg[3].dst"}};
static_assert(FPD_EMA_MAX_SEG == 4, "seg_names has a row per segment");

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
    *blocks = grid_for(a.copy_n);
    for (int s = 0; s < a.nseg; ++s) {
        const fpd_ema_seg_t& g = a.seg[s];
        if (const int rc = require_flat_n(seg_names[s][0], g.n)) return rc;
        FPD_REQUIRE(g.n == 0 || (g.src != nullptr && g.dst != nullptr), "ema: segment %d: null pointer with n = %lld", s, (long long)g.n);
        int seg_blocks = 0;
        flat_geometry(g.n, (uintptr_t)g.src | (uintptr_t)g.dst, nullptr, &nvec[s], &seg_blocks);
        *blocks = *blocks > seg_blocks ? *blocks : seg_blocks;
        if (g.n > 0) {
            r[nr++] = range_of(g.src, 4 * (uint64_t)g.n, false, seg_names[s][1]);
            r[nr++] = range_of(g.dst, 4 * (uint64_t)g.n, true, seg_names[s][2]);
        }
    }
    if (a.copy_n > 0) {
        r[nr++] = range_of(a.copy_src, 8 * (uint64_t)a.copy_n, false, "copy_src");
        r[nr++] = range_of(a.copy_dst, 8 * (uint64_t)a.copy_n, true, "copy_dst");
    }
    r[nr++] = range_of(a.updates_dev, 8, true, "updates_dev");
    return require_disjoint("ema", r, nr);
}

int fpd_ema_launch(const fpd_ema_t& a, hipStream_t st) {
    ema_vecs v = {};
    int blocks = 0;
    const int rc = fpd_ema_geometry_of(a, &blocks, v.nvec);
    if (rc) return rc;
    FPD_LAUNCH(ema_kernel, dim3(blocks), dim3(256), 0, st, a, v);
    FPD_LAUNCH(tick_kernel, dim3(1), dim3(1), 0, st, a.updates_dev);
    return 0;
}
