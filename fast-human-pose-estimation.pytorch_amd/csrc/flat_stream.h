// What the streaming launches over flat fp32 arenas share (loss_adam.hip sgd_kernel, adamw.hip, ema.hip, grad_clip.hip,
// grad_accum.hip): on the device one grid-stride "vectors, then tail" walk that a kernel hands its per-element update to, and
// the one-thread counter tick; on the host the byte ranges and their disjointness check, the range check of n and the launch
// geometry.  The arithmetic is not here: it stays in each unit's *_math.h, which a host build checks against numpy.
#pragma once
#include <type_traits>

#include "common.h"
#include "conv_dispatch.h"

namespace {

// ---- device ----------------------------------------------------------------------------------------------------------

struct flat_out { float* p; };                               // an arena the update only writes (it is never loaded)
template <int W> struct alignas(4 * W) flat_vals { float e[W]; };      // W = 4: one 16-byte vector, W = 1: one element

// The thread's index in the grid and the grid's size.  (The builtin, not blockDim.x: outside a __global__ function the latter is
// compiled for blocks of unequal sizes, a select and a vector load in front of every kernel's first trip.)
__device__ __forceinline__ int64_t flat_tid() { return (int64_t)blockIdx.x * __builtin_amdgcn_workgroup_size_x() + threadIdx.x; }
__device__ __forceinline__ int64_t flat_nthr() { return (int64_t)gridDim.x * __builtin_amdgcn_workgroup_size_x(); }

// W values of an arena from element i on.  The arena's type says what the walk does with it: `const float*` is read, `float*`
// is read and written back, flat_out is written only.
template <int W, typename P>
__device__ __forceinline__ flat_vals<W> flat_load(P a, int64_t i) {
    if constexpr (std::is_same_v<P, flat_out>) return {};
    else return *reinterpret_cast<const flat_vals<W>*>(a + i);
}
template <int W, typename P>
__device__ __forceinline__ void flat_store(P a, int64_t i, const flat_vals<W>& v) {
    if constexpr (std::is_same_v<P, flat_out>) *reinterpret_cast<flat_vals<W>*>(a.p + i) = v;
    else if constexpr (!std::is_const_v<std::remove_pointer_t<P>>) *reinterpret_cast<flat_vals<W>*>(a + i) = v;
}
// the bf16 working copy of the same elements: one 8-byte store of two packed pairs, or one element
__device__ __forceinline__ void flat_store_lp(bf16_t* lp, int64_t i, const flat_vals<4>& v) {
    *reinterpret_cast<uint2*>(lp + i) = make_uint2(f2bf_pk(v.e[0], v.e[1]), f2bf_pk(v.e[2], v.e[3]));
}
__device__ __forceinline__ void flat_store_lp(bf16_t* lp, int64_t i, const flat_vals<1>& v) { lp[i] = f2bf(v.e[0]); }

// Elements i .. i + W - 1, i a multiple of W: every arena's values are loaded, f(element index, one float& per arena, in the
// order given) runs on each element in index order, and what is writable goes back.  lp (may be null): the bf16 copy of the
// FIRST arena's new values.  The index is formed as i | e so that the compiler sees that the W elements share (i | e) >> k
// for 2^k >= W: a functor that reads a bit mask by the element's index (adamw.hip) costs one load per vector, not W.
template <int W, typename F, typename A0, typename... A>
__device__ __forceinline__ void flat_trip(int64_t i, bf16_t* lp, F& f, A0 a0, A... a) {
    [&](auto v0, auto... v) {
#pragma unroll
        for (int e = 0; e < W; ++e) f(i | e, v0.e[e], v.e[e]...);
        flat_store<W>(a0, i, v0);
        (flat_store<W>(a, i, v), ...);
        if (lp) flat_store_lp(lp, i, v0);
    }(flat_load<W>(a0, i), flat_load<W>(a, i)...);
}

// One grid-stride walk over the elements [0, n) of same-sized arenas: nvec 16-byte vectors (0 when an arena is off the 16-byte
// grid, flat_geometry() below), then the elements [4 nvec, n) one by one.  One writer per element.
template <typename F, typename... A>
__device__ __forceinline__ void flat_walk(int64_t n, int64_t nvec, bf16_t* lp, F f, A... a) {
    const int64_t tid = flat_tid(), nthr = flat_nthr();
    for (int64_t i = tid; i < nvec; i += nthr) flat_trip<4>(4 * i, lp, f, a...);
    for (int64_t i = 4 * nvec + tid; i < n; i += nthr) flat_trip<1>(i, lp, f, a...);
}

// The step / update counter moves in a launch of its own behind the one that reads it: every thread of that launch forms its
// coefficients from the counter, and no block may see it move.
__global__ void tick_kernel(int64_t* counter) { *counter += 1; }

// ---- host: pure, nothing is dereferenced -----------------------------------------------------------------------------

struct byte_range { uintptr_t lo, hi; bool written; const char* name; };
inline byte_range range_of(const void* p, uint64_t bytes, bool written, const char* name) {
    return {(uintptr_t)p, (uintptr_t)p + (uintptr_t)bytes, written, name};
}

// A range the launch writes must not share a byte with any other; two that are only read may alias.
inline int require_disjoint(const char* unit, const byte_range* r, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            FPD_REQUIRE(!((r[i].written || r[j].written) && r[i].lo < r[j].hi && r[j].lo < r[i].hi),
                        "%s: %s overlaps %s (a written range must not alias another)", unit, r[i].name, r[j].name);
    return 0;
}

// n is a count of fp32 elements whose byte ranges can be formed: `what` names it in the message ("adamw", "ema: segment 1")
inline int require_flat_n(const char* what, int64_t n) {
    FPD_REQUIRE(n >= 0, "%s: n = %lld is negative", what, (long long)n);
    FPD_REQUIRE(n < ((int64_t)1 << 60), "%s: n = %lld is too large", what, (long long)n);
    return 0;
}

// ptr_bits: the OR of the fp32 arenas' addresses.  All on the 16-byte grid (and the bf16 copy, when there is one, on the 8-byte
// grid): nvec = n / 4 vectors and n % 4 tail elements; else every element goes through the tail.  -> the grid that covers the
// longer of the two loops.
inline void flat_geometry(int64_t n, uintptr_t ptr_bits, const void* lp, int64_t* nvec, int* blocks) {
    const bool aligned = (ptr_bits & 15) == 0 && ((uintptr_t)lp & 7) == 0;
    *nvec = aligned ? n / 4 : 0;
    const int64_t rest = n - 4 * *nvec;
    *blocks = grid_for(*nvec > rest ? *nvec : rest);
}

}  // namespace
