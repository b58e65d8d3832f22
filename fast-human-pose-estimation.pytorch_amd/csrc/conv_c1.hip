// conv_c1: STREAMING 1x1 convolution for the big maps of the student chain (bf16, C, K in {32, 64, 128}, N*H*W a multiple of
// 32): forward (BatchNorm+ReLU prologue, bias / residual, batch statistics of the result) and the BatchNorm-backward data
// gradient (ReLU mask of epi_x + the two sums), optionally evaluating a folded BN-backward apply on its operand (fold_x) and
// forming the forward convolution's weight / bias gradient in the same launch (wg_partial).  Same contract as conv_pp /
// conv_tile (fpd_conv_t); round 6.
//
// Why a third kernel.  Round 5 found conv_pp's tile loops bound by instruction ISSUE: 400-1 200 vector instructions per wave
// and 128-pixel tile around 8-16 MFMAs, three block barriers per tile (nine serial phases in the data gradients, one block
// per CU), every element passing through the LDS twice as fp32.  A 1x1 convolution has no halo, so nothing has to be shared
// between waves at all:
//   * a WAVE owns a 32-pixel tile outright -- all K output channels of it.  It brings the tile as whole 1 KB lines (lane l
//     always holds the same 8 channels, so BN scale / shift, the coefficients of a folded apply, the epilogue tables and the
//     statistics accumulators are registers, loaded once per block), applies the prologue, writes the operand into its
//     PRIVATE LDS tile and reads its MFMA fragments from there; the weights sit in the LDS once per block (XOR-swizzled);
//   * the transposed MFMA (weights first) leaves a lane with 4 consecutive channels of one pixel: + residual + bias in fp32,
//     ONE rounding, an 8-byte LDS store into the wave's bf16 output tile -- which is read back as whole 16-byte vectors of 8
//     channels for everything that is per channel (statistics; ReLU mask of the data gradient, which commutes with the
//     rounding; the forward operand a(u) of the fused weight gradient) and leaves as 1 KB global stores;
//   * no barrier in the tile loop (a wave's LDS operations execute in order): eight waves of a block drift apart and fill
//     each other's latencies.  Only the fused weight gradient exchanges data: after a ROUND (8 waves x 32 pixels) a wave
//     multiplies ITS 32x32 tile of dW over the 256 pixels of all eight tiles (dy and a(u) through transposing LDS reads:
//     two barriers per round), so no cross-wave reduction is ever needed and a block writes one slab at the end.
// Instructions per wave and 256-pixel round (isa_report): see DESIGN.md section 5.
//
// Replaces the same reference calls as conv_pp (nn.Conv2d 1x1 + BatchNorm2d + ReLU and their autograd,
// /root/reference/lib/models/hourglass.py:18-52, 134-137).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "conv_dispatch.h"
#include "conv_stream.h"
#include "mfma_frag.h"

namespace {

constexpr int C1_NW = 8;                                 // waves per block = tiles per round

// C, K: channels in / out of THIS launch.  BWD: BNRELU_BWD epilogue (no bias, no residual, no prologue BN).  FOLD (BWD only):
// the operand is a folded BN-backward apply (fold_x).  WG (BWD only): also the weight / bias gradient of the forward
// convolution this launch is the data gradient of.  SKIP (forward only, no RES): a second 1x1 source of C channels (fpd_conv_t.x2,
// the downsample branch of a Bottleneck) whose rounded result is the residual: its weights and bias sit behind the first ones.
template <int C, int K, bool BWD, bool WG, bool SKIP = false>
struct C1Geo {
    static constexpr int CV = C / 8, KV = K / 8;         // 16-byte chunks per operand / output pixel
    static constexpr int NV = C / 16, NK = K / 16;       // operand / output vectors per lane and tile (32 px * CV / 64)
    static constexpr int KT = K / 32, KS = C / 16;       // 32-channel output tiles, 16-channel reduction steps
    static constexpr int PXA = C * 2 + 16, PXO = K * 2 + 16;     // pixel pitch of the operand / output tile (bytes)
    static constexpr int TILE_A = 32 * PXA, TILE_O = 32 * PXO;
    // (only the fused weight gradient reads the operand tile after the products: without it the output tile takes its place)
    static constexpr int WAVE_LDS = WG ? TILE_A + TILE_O : (TILE_A > TILE_O ? TILE_A : TILE_O);
    static constexpr int FLUSH = C1_NW * 64 * 16 * 4 + C1_NW * K * 4 + 8 * 2 * K * 8;      // statistics records + common shifts + partial sums
    static constexpr int REGION = C1_NW * WAVE_LDS > FLUSH ? C1_NW * WAVE_LDS : FLUSH;
    static constexpr int TABLES = (2 * C + (BWD ? 3 * C + 4 * K : 0) + K + (SKIP ? K : 0)) * 4;
    static constexpr int LDS = TABLES + (SKIP ? 2 : 1) * K * C * 2 + REGION;
    static constexpr int NT = (C / 32) * (K / 32);       // 32x32 tiles of dW
    static constexpr int NTW = NT / C1_NW;               // ... per wave
    static_assert(!WG || (BWD && NT % C1_NW == 0 && NTW >= 1), "fused weight gradient: every wave owns whole tiles of dW");
    static_assert(64 % CV == 0 && 64 % KV == 0, "a lane keeps its channel chunk");
    static_assert(!SKIP || (!BWD && !WG && K == 2 * C), "second source: forward launches C -> 2C only");
};

// the compiler may not move LDS accesses across the phases of a tile: the phases of ONE wave communicate through its private
// tiles without a barrier (a wave's LDS operations execute in order), with accesses of different vector types
// (and no arithmetic either: hipcc fills the shadow of the MFMAs with the NEXT phase's unpacking of every vector in flight,
//  which costs more registers than the kernel has; the other wave of the SIMD is what runs beside the matrix pipe)
#define C1_PHASE() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

#ifdef FPD_C1_TIMING      // probe build only: cycle stamps of waves 0 and 7 of two blocks at the phase boundaries, printed by the kernel
#define C1_STAMP() do { if (lane == 0 && (wave == 0 || wave == 7) && c1_ns < 40) c1_stamp[(wave ? 40 : 0) + c1_ns++] = clock64(); } while (0)
#else
#define C1_STAMP() do { } while (0)
#endif

template <int C, int K, bool BWD, bool FOLD, bool WG, bool RES, bool SKIP>
__device__ __forceinline__ void c1_body(const fpd_conv_t& a, const int bi, const int nblk) {
    static_assert(!(SKIP && RES), "the second source IS the residual");
    using G = C1Geo<C, K, BWD, WG, SKIP>;
    constexpr int CV = G::CV, KV = G::KV, NV = G::NV, NK = G::NK, KT = G::KT, KS = G::KS, PXA = G::PXA, PXO = G::PXO;
    constexpr int RPB = CV >= 16 ? 1 : 16 / CV;           // weight rows per 256-byte bank row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.N * a.H * a.W;
    const int ntile = M >> 5;                             // (M % 32 == 0: checked by the host)
    const int nround = (ntile + C1_NW - 1) / C1_NW;
    const int r_beg = fpd_cut(bi, nround, nblk), r_end = fpd_cut(bi + 1, nround, nblk);

    float* s_scale = reinterpret_cast<float*>(smem);      // [C] prologue BN
    float* s_shift = s_scale + C;                         // [C]
    float* s_fold = s_shift + C;                          // BWD: [3][C] coefficients of a folded BN-backward apply
    float* s_epi = s_fold + (BWD ? 3 * C : 0);            // BWD: [4][K] scale, shift, mean, invstd of epi_bn
    float* s_bias = s_epi + (BWD ? 4 * K : 0);            // [K]
    float* s_bias2 = s_bias + K;                          // SKIP: [K] bias of the second source
    unsigned char* sW = reinterpret_cast<unsigned char*>(s_bias + K + (SKIP ? K : 0));     // [K][C] bf16, 16-byte chunk c of row n at c ^ sw(n)
    unsigned char* sW2 = sW + K * C * 2;                  // SKIP: the second source's weights, same layout
    unsigned char* sT = sW + (SKIP ? 2 : 1) * K * C * 2;  // the waves' tiles
    unsigned char* tA = sT + wave * G::WAVE_LDS;          // operand tile [32 px][PXA]
    unsigned char* tO = WG ? tA + G::TILE_A : tA;         // output tile [32 px][PXO] (no fused weight gradient: the operand tile is dead by then)

    const bf16_t* __restrict__ x = reinterpret_cast<const bf16_t*>(a.x);
    const bf16_t* __restrict__ w = reinterpret_cast<const bf16_t*>(a.w);
    const bf16_t* __restrict__ x2 = reinterpret_cast<const bf16_t*>(a.x2);      // SKIP
    const bf16_t* __restrict__ w2 = reinterpret_cast<const bf16_t*>(a.w2);
    bf16_t* y = reinterpret_cast<bf16_t*>(a.y);           // (the residual may alias it)
    const bf16_t* res = reinterpret_cast<const bf16_t*>(a.residual);
    const bf16_t* ex = reinterpret_cast<const bf16_t*>(a.epi_x);
    // (a launch whose OTHER convolution folds: u is loaded from the operand itself and ignored -- no conditional loads)
    const bf16_t* __restrict__ fx = reinterpret_cast<const bf16_t*>(a.fold_x != nullptr ? a.fold_x : a.x);
    const bool fold = FOLD && a.fold_x != nullptr;        // (FOLD: some convolution of the launch folds; this one may not)
    bf16_t* fo = fold ? reinterpret_cast<bf16_t*>(a.fold_out) : nullptr;
    const bool has_bn = !BWD && a.bn.mode != FPD_BN_NONE;
    constexpr bool has_res = RES;                         // (forward only; a template parameter: no conditional loads)
    const bool want_stats = BWD || a.out_stats != nullptr;
    const bool wg = WG && a.wg_partial != nullptr;
    const bool wg_bias = wg && a.wg_bias;
#ifdef FPD_C1_TIMING
    long long* c1_stamp = reinterpret_cast<long long*>(smem + G::LDS);      // [2][40] behind everything (the probe build asks for 1 KB more)
    int c1_ns = 0;
#endif
    C1_STAMP();

    // ---- prologue: the table chains requested before the long loads (StreamTables, conv_stream.h) ----
    StreamTables<C, K, BWD, SKIP> tab;
    tab.request(a, tid, has_bn, fold);
    __builtin_amdgcn_sched_barrier(0);

    // ---- the tile's vectors: vector i of a lane is 16 bytes at (tile base) + (i * 64 + lane) * 16 -- whole 1 KB lines ----
    uint4 rx[NV];                                         // operand (fold: the masked gradient g)
    uint4 ru[FOLD ? NV : 1];                              // fold: the BN input u
    uint4 rr[SKIP ? 1 : NK];                              // forward: residual; backward: epi_x
    uint4 rx2[SKIP ? NV : 1];                             // SKIP: the second source (C channels: half the registers of the residual)
    auto load_x2 = [&](int t) {
        const uint4* px = reinterpret_cast<const uint4*>(x2) + ((size_t)t * 32 * CV + lane);
#pragma unroll
        for (int i = 0; i < (SKIP ? NV : 1); ++i) rx2[i] = px[i * 64];
    };
    auto load_x = [&](int t) {
        const uint4* px = reinterpret_cast<const uint4*>(x) + ((size_t)t * 32 * CV + lane);
#pragma unroll
        for (int i = 0; i < NV; ++i) rx[i] = px[i * 64];
        if constexpr (FOLD) {
            const uint4* pu = reinterpret_cast<const uint4*>(fx) + ((size_t)t * 32 * CV + lane);
#pragma unroll
            for (int i = 0; i < NV; ++i) ru[i] = pu[i * 64];
        }
    };
    auto load_r = [&](int t) {                            // (callers test has_res in forward mode)
        const uint4* pr = reinterpret_cast<const uint4*>(BWD ? ex : res) + ((size_t)t * 32 * KV + lane);
#pragma unroll
        for (int i = 0; i < (SKIP ? 1 : NK); ++i) rr[i] = pr[i * 64];
    };
    int tile = r_beg * C1_NW + wave;
    {
        // requested in the order they are needed: tables (above), weights -- the first barrier waits for both --, then the
        // first tile (100+ KB per block: at the chip's ~12 bytes per cycle and CU it takes 6-11 k cycles to arrive; stamps)
        constexpr int NWV = (K * CV + 511) / 512;         // weight vectors per thread
        uint4 rw[NWV], rw2[SKIP ? NWV : 1];
#pragma unroll
        for (int i = 0; i < NWV; ++i) {
            const int v = tid + i * 512;
            rw[i] = make_uint4(0, 0, 0, 0);
            if (v < K * CV) rw[i] = *reinterpret_cast<const uint4*>(w + (size_t)v * 8);
            if constexpr (SKIP) {
                rw2[i] = make_uint4(0, 0, 0, 0);
                if (v < K * CV) rw2[i] = *reinterpret_cast<const uint4*>(w2 + (size_t)v * 8);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            // (unconditionally, a wave without a tile re-reads the last one: behind a branch hipcc waits for EVERY load in
            //  flight -- vmcnt(0) -- before the weights go to the LDS, i.e. the first barrier waited for the whole first tile)
            const int t0 = min(tile, ntile - 1);
            if constexpr (SKIP) load_x2(t0);             // (needed first)
            load_x(t0);
            if constexpr (BWD || has_res) load_r(t0);
        }
        __builtin_amdgcn_sched_barrier(0);
        tab.resolve(a, tid, M, bi == 0, s_scale, s_shift, s_fold, s_epi, s_bias, s_bias2);
#pragma unroll
        for (int i = 0; i < NWV; ++i) {
            const int v = tid + i * 512;
            if (v < K * CV) {
                const int k = v / CV, ch = v % CV;
                const int sw = (k / RPB) & (CV - 1);
                *reinterpret_cast<uint4*>(sW + (k * CV + (ch ^ sw)) * 16) = rw[i];
                if constexpr (SKIP) *reinterpret_cast<uint4*>(sW2 + (k * CV + (ch ^ sw)) * 16) = rw2[i];
            }
        }
    }
    C1_STAMP();
    __syncthreads();                                      // tables + weights visible
    C1_STAMP();

    // ---- per-lane constants: the 8 channels of this lane's operand / output chunk ----
    const int cch = lane % CV, kch = lane % KV;           // chunk of the operand / output pixel this lane always holds
    const int pxa0 = lane / CV, pxo0 = lane / KV;         // its pixel in vector 0 (vector i: + i * 64 / CV)
    f32x2 p_sc[4], p_sh[4];                               // forward BN scale / shift, as pairs
    if (has_bn) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            p_sc[e] = *reinterpret_cast<const f32x2*>(s_scale + cch * 8 + 2 * e);
            p_sh[e] = *reinterpret_cast<const f32x2*>(s_shift + cch * 8 + 2 * e);
        }
    }
    // (the data gradients re-read their per-channel tables from the LDS in the phase that uses them: the registers are
    //  needed for the accumulators and the vectors in flight)
    const short relu_floor = a.bn.relu ? (short)0 : (short)-32768;
    const short epi_floor = a.epi_bn.relu ? (short)0 : (short)-32768;
    const float relu_gate = a.epi_bn.relu ? 0.f : -3.4e38f;
    f32x2 F1[4], F2[4], CS[4];                            // statistics partials / common shift of this lane's 8 output channels
#pragma unroll
    for (int e = 0; e < 4; ++e) { F1[e] = f32x2{0.f, 0.f}; F2[e] = f32x2{0.f, 0.f}; CS[e] = f32x2{0.f, 0.f}; }
    const int wsw = (l31 / RPB) & (CV - 1);               // swizzle of this lane's weight rows (row = kt * 32 + l31)
    f32x16 wacc[WG ? G::NTW : 1], bacc[WG ? G::NTW : 1];  // WG: this wave's tiles of dW / of the bias gradient
#pragma unroll
    for (int j = 0; j < (WG ? G::NTW : 1); ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) { wacc[j][e] = 0.f; bacc[j][e] = 0.f; }

    // ---- 1. operand: prologue on the way into the wave's tile ----
    auto stage = [&](const int t, auto modec) {
        constexpr int MODE = decltype(modec)::value;       // 0 = raw operand, 1 = BatchNorm(+ReLU) prologue, 2 = folded BN-backward apply
        f32x2 f_a[4], f_b[4], f_d[4];                     // fold coefficients of this lane's 8 channels
        if constexpr (MODE == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f_a[e] = *reinterpret_cast<const f32x2*>(s_fold + cch * 8 + 2 * e);
                f_b[e] = *reinterpret_cast<const f32x2*>(s_fold + C + cch * 8 + 2 * e);
                f_d[e] = *reinterpret_cast<const f32x2*>(s_fold + 2 * C + cch * 8 + 2 * e);
            }
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            uint4 val = rx[i];
            if constexpr (MODE == 2) {
                const uint4 uu = ru[i];
                const unsigned gw[4] = {val.x, val.y, val.z, val.w}, uw[4] = {uu.x, uu.y, uu.z, uu.w};
                unsigned ow[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const f32x2 tt = __builtin_elementwise_fma(f_b[e], bf2_unpack(uw[e]), f_d[e]);
                    ow[e] = bf2_pack(__builtin_elementwise_fma(f_a[e], bf2_unpack(gw[e]), tt));
                }
                val = make_uint4(ow[0], ow[1], ow[2], ow[3]);
            } else if constexpr (MODE == 1) {
                val.x = bf2_floor(bf2_pack(__builtin_elementwise_fma(bf2_unpack(val.x), p_sc[0], p_sh[0])), relu_floor);
                val.y = bf2_floor(bf2_pack(__builtin_elementwise_fma(bf2_unpack(val.y), p_sc[1], p_sh[1])), relu_floor);
                val.z = bf2_floor(bf2_pack(__builtin_elementwise_fma(bf2_unpack(val.z), p_sc[2], p_sh[2])), relu_floor);
                val.w = bf2_floor(bf2_pack(__builtin_elementwise_fma(bf2_unpack(val.w), p_sc[3], p_sh[3])), relu_floor);
            }
            rx[i] = val;
            *reinterpret_cast<uint4*>(tA + (pxa0 + i * (64 / CV)) * PXA + cch * 16) = val;
        }
        if (MODE == 2 && fo != nullptr) {                 // the evaluated operand has other readers: written out once
            uint4* po = reinterpret_cast<uint4*>(fo) + ((size_t)t * 32 * CV + lane);
#pragma unroll
            for (int i = 0; i < NV; ++i) po[i * 64] = rx[i];
        }
    };
    // SKIP: the second source's lines go into the tile raw (same geometry as the operand: C channels)
    auto stage2 = [&]() {
#pragma unroll
        for (int i = 0; i < (SKIP ? NV : 1); ++i)
            *reinterpret_cast<uint4*>(tA + (pxa0 + i * (64 / CV)) * PXA + cch * 16) = make_uint4(rx2[i].x, rx2[i].y, rx2[i].z, rx2[i].w);
    };
    // ---- 3. + residual + bias in fp32, ONE rounding, into the wave's bf16 output tile (lane: pixel l31, channels
    //         kt * 32 + 8 q + 4 hh .. + 3); sb: the bias table (SKIP: of the source being finished) ----
    auto finish = [&](const f32x16& accv, const int kt, auto resc, const float* sb) {
        constexpr bool HASRES = decltype(resc)::value;
        {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned char* p = tO + l31 * PXO + (kt * 32 + 8 * q + 4 * hh) * 2;
                f32x2 v0 = {accv[4 * q], accv[4 * q + 1]}, v1 = {accv[4 * q + 2], accv[4 * q + 3]};
                if constexpr (!BWD) {
                    if constexpr (HASRES) {
                        const uint2 r2 = *reinterpret_cast<const uint2*>(p);
                        v0 += bf2_unpack(r2.x);
                        v1 += bf2_unpack(r2.y);
                    }
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(sb + kt * 32 + 8 * q + 4 * hh);
                    v0 += f32x2{b4[0], b4[1]};
                    v1 += f32x2{b4[2], b4[3]};
                }
                *reinterpret_cast<uint2*>(p) = make_uint2(bf2_pack(v0), bf2_pack(v1));
            }
        }
    };
    // ---- 4. per channel: whole vectors of 8 channels again (vector i: pixel pxo0 + i * 64 / KV, chunk kch) ----
    auto perchan = [&](const int t, const bool first, auto statc) {
        constexpr bool STATS = decltype(statc)::value;
        uint4* py = reinterpret_cast<uint4*>(y) + ((size_t)t * 32 * KV + lane);
        EpiTab et;                                        // BWD: epilogue BN of this lane's 8 output channels
        if constexpr (BWD) epi_tab_read<K>(s_epi, kch, et);
        if (!BWD && STATS && first)                       // common shift of the wave's shifted sums: the value of its first pixel
            bf2_unpack4(*reinterpret_cast<const uint4*>(tO + kch * 16), CS);      // (every lane of a chunk reads it)
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            unsigned char* p = tO + (pxo0 + i * (64 / KV)) * PXO + kch * 16;
            const uint4 o4 = *reinterpret_cast<const uint4*>(p);
            unsigned ow[4] = {o4.x, o4.y, o4.z, o4.w};
            if constexpr (BWD) {
                const unsigned xw[4] = {rr[i].x, rr[i].y, rr[i].z, rr[i].w};
                unsigned aw[4];                           // WG: the forward operand a(u) takes the gradient's place in the tile
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const f32x2 z = epi_bwd_pair(ow[e], xw[e], et, e, relu_gate, F1[e], F2[e]);
                    if constexpr (WG) aw[e] = bf2_floor(bf2_pack(z), epi_floor);     // as the forward convolution staged it
                }
                if constexpr (WG) *reinterpret_cast<uint4*>(p) = make_uint4(aw[0], aw[1], aw[2], aw[3]);
            } else if constexpr (STATS) epi_fwd_step(ow, CS, F1, F2);
            py[i * 64] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
            if constexpr (BWD || STATS) epi_sums_fence(F1, F2);
        }
    };

    // ---- 5. WG: this wave's tiles of dW over the 256 pixels of the round (dy^T and a(u) through transposing reads).  A full
    //         round is unrolled with the fragments of tile s + 1 requested before the products of tile s (stamps of the
    //         rolled loop: 5-6.7 k cycles per round for 16-32 MFMAs -- every pair of tiles waited for its LDS reads) ----
    auto wg_frags = [&](const int s, bf16x8 (&af)[2][WG ? G::NTW : 1], bf16x8 (&bfr)[2][WG ? G::NTW : 1]) {
        const bf16_t* dyT = reinterpret_cast<const bf16_t*>(sT + s * G::WAVE_LDS);
        const bf16_t* aT = reinterpret_cast<const bf16_t*>(sT + s * G::WAVE_LDS + G::TILE_A);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int j = 0; j < (WG ? G::NTW : 1); ++j) {
                const int tw = wave + C1_NW * j, ci = tw / KT, ko = tw % KT;
                af[h][j] = tr_frag_bf16(dyT, PXA / 2, h * 16, ci * 32, lane);
                bfr[h][j] = tr_frag_bf16(aT, PXO / 2, h * 16, ko * 32, lane);
            }
        }
    };
    auto wg_round = [&](const int round, auto biasc) {
        constexpr bool BIAS = decltype(biasc)::value;      // this wave owns tiles with ko == 0: the bias gradient rides along
        const bf16x8 ones = {(__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f, (__bf16)1.f};
        bf16x8 af[2][2][WG ? G::NTW : 1], bfr[2][2][WG ? G::NTW : 1];      // [buffer][pixel half][tile]
        auto mult = [&](const int b) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int j = 0; j < (WG ? G::NTW : 1); ++j) {
                    wacc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[b][h][j], bfr[b][h][j], wacc[j], 0, 0, 0);
                    if constexpr (BIAS) bacc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[b][h][j], ones, bacc[j], 0, 0, 0);
                }
            }
        };
        if (round * C1_NW + C1_NW <= ntile) {
            wg_frags(0, af[0], bfr[0]);
#pragma unroll
            for (int s = 0; s < C1_NW; ++s) {
                if (s + 1 < C1_NW) wg_frags(s + 1, af[(s + 1) & 1], bfr[(s + 1) & 1]);
                mult(s & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll 1
            for (int s = 0; s < C1_NW; ++s) {
                if (round * C1_NW + s < ntile) {
                    wg_frags(s, af[0], bfr[0]);
                    mult(0);
                }
            }
        }
    };

    // =========================== the round loop ===========================
    bool first = true;
    for (int round = r_beg; round < r_end; ++round) {
        tile = round * C1_NW + wave;
        const bool live = tile < ntile;                   // (wave-uniform)
        const bool pf = round + 1 < r_end && tile + C1_NW < ntile;      // a next tile to prefetch
        if (live) {
            bf16x8 bf2[SKIP ? KS : 1];
            if constexpr (SKIP) {
                // ---- 0. the second source passes through the tile first: raw lines in, fragments out, then the operand proper
                //         takes the tile over (the output tile aliases it: both sets of fragments are registers before the first
                //         finish) ----
                stage2();
                if (pf) load_x2(tile + C1_NW);
                C1_PHASE();
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) bf2[kk] = *reinterpret_cast<const bf16x8*>(tA + l31 * PXA + kk * 32 + hh * 16);
                C1_PHASE();
            }
            if (FOLD && fold) { if constexpr (FOLD) stage(tile, std::integral_constant<int, 2>{}); }
            else if (has_bn) { if constexpr (!BWD) stage(tile, std::integral_constant<int, 1>{}); }
            else stage(tile, std::integral_constant<int, 0>{});
            if (pf) load_x(tile + C1_NW);                 // the next tile's vectors take the registers over
            C1_PHASE();
            C1_STAMP();
            // ---- 2. the products: D[k][px] = sum_c W[k][c] * opnd[px][c]; a lane gets 4 consecutive channels of pixel l31 ----
            bf16x8 bf[KS];
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) bf[kk] = *reinterpret_cast<const bf16x8*>(tA + l31 * PXA + kk * 32 + hh * 16);
            if constexpr (has_res) {                       // the residual goes through the output tile (after the fragments are read)
                C1_PHASE();
#pragma unroll
                for (int i = 0; i < NK; ++i)
                    *reinterpret_cast<uint4*>(tO + (pxo0 + i * (64 / KV)) * PXO + kch * 16) = make_uint4(rr[i].x, rr[i].y, rr[i].z, rr[i].w);
                C1_PHASE();
            }
            if constexpr (SKIP) {
                // skip = round(W2 x2 + bias2) into the output tile -- what the plain launch of the downsample convolution stores --
                // and the products below add it like any residual
                C1_PHASE();
#pragma unroll
                for (int k0 = 0; k0 < KT; k0 += 2) {
                    f32x16 acc0, acc1;
#pragma unroll
                    for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
                    const unsigned char* wrow0 = sW2 + (k0 * 32 + l31) * (C * 2);
#pragma unroll
                    for (int kk = 0; kk < KS; ++kk) {
                        const bf16x8 wf0 = *reinterpret_cast<const bf16x8*>(wrow0 + ((2 * kk + hh) ^ wsw) * 16);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf0, bf2[kk], acc0, 0, 0, 0);
                        const bf16x8 wf1 = *reinterpret_cast<const bf16x8*>(wrow0 + 32 * (C * 2) + ((2 * kk + hh) ^ wsw) * 16);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf1, bf2[kk], acc1, 0, 0, 0);
                    }
                    finish(acc0, k0, std::false_type{}, s_bias2);
                    finish(acc1, k0 + 1, std::false_type{}, s_bias2);
                }
                C1_PHASE();
            }
            // two 32-channel tiles of the output at a time: the accumulators of one pair are finished (step 3) while the next
            // pair multiplies
#pragma unroll
            for (int k0 = 0; k0 < KT; k0 += 2) {
                f32x16 acc0, acc1;
#pragma unroll
                for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
                const unsigned char* wrow0 = sW + (k0 * 32 + l31) * (C * 2);
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    const bf16x8 wf0 = *reinterpret_cast<const bf16x8*>(wrow0 + ((2 * kk + hh) ^ wsw) * 16);
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf0, bf[kk], acc0, 0, 0, 0);
                    if (k0 + 1 < KT) {
                        const bf16x8 wf1 = *reinterpret_cast<const bf16x8*>(wrow0 + 32 * (C * 2) + ((2 * kk + hh) ^ wsw) * 16);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf1, bf[kk], acc1, 0, 0, 0);
                    }
                }
                finish(acc0, k0, std::integral_constant<bool, has_res || SKIP>{}, s_bias);
                if (k0 + 1 < KT) finish(acc1, k0 + 1, std::integral_constant<bool, has_res || SKIP>{}, s_bias);
            }
            if constexpr (!BWD && has_res) { if (pf) load_r(tile + C1_NW); }
            C1_PHASE();
            C1_STAMP();
            if (want_stats) perchan(tile, first, std::true_type{}); else perchan(tile, first, std::false_type{});
            if (BWD && pf) load_r(tile + C1_NW);
            C1_PHASE();
            C1_STAMP();
            first = false;
        }
        if (WG) {
            __syncthreads();                              // the eight tiles of the round: dy and a(u) complete
            if (wg) {
                // (whether this wave also multiplies for the bias gradient is decided once: a branch per MFMA otherwise)
                if (wg_bias && (wave % KT) == 0) wg_round(round, std::true_type{}); else wg_round(round, std::false_type{});
            }
            __syncthreads();                              // tiles free for the next round
            C1_STAMP();
        }
    }
    C1_STAMP();

    // ---- WG: this block's slab -- every wave stores the tiles of dW it owns (fpd_wgrad_reduce adds the slabs in order) ----
    if (WG && wg) {
        float* slab = a.wg_partial + (size_t)bi * a.wg_stride;
#pragma unroll
        for (int j = 0; j < (WG ? G::NTW : 1); ++j) {
            const int tw = wave + C1_NW * j, ci = tw / KT, ko = tw % KT;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = ci * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                slab[(size_t)row * K + ko * 32 + l31] = wacc[j][e];
                if (wg_bias && ko == 0 && l31 == 0) slab[(size_t)C * K + row] = bacc[j][e];
            }
        }
    }

    // ---- statistics: one flush per block (stream_stats_flush, conv_stream.h) ----
    if (want_stats)
        stream_stats_flush<C1_NW, K, BWD>(reinterpret_cast<float*>(sT), BWD ? a.epi_stats : a.out_stats, F1, F2, CS, wave, lane, tid, [&](const int wv) {
            // tiles wave wv has processed: rounds r of this block with r * 8 + wv < ntile
            const int last = (ntile - 1 - wv) >= 0 ? (ntile - 1 - wv) / C1_NW : -1;
            const int hi = min(r_end - 1, last);
            return hi >= r_beg ? hi - r_beg + 1 : 0;
        });
#ifdef FPD_C1_TIMING
    C1_STAMP();
    if (lane == 0 && (wave == 0 || wave == 7)) c1_stamp[(wave ? 40 : 0) + 39] = c1_ns;
    __syncthreads();
    if (tid == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2 + 1)) {
        // entry | tables + weights stored | barrier | per tile: staged (+ next requested), products + finish, per-channel + stores (WG: + round) | loop end | flush
        // (one printf per row: concurrent printfs interleave)
        for (int wv = 0; wv < 2; ++wv) {
            const long long* sp = c1_stamp + wv * 40;
            const long long t0 = c1_stamp[0];
            long long d[16];
            for (int q = 0; q < 16; ++q) d[q] = q < (int)sp[39] ? sp[q] - t0 : -1;
            printf("conv_c1 C=%d K=%d bwd %d fold %d wg %d blk %d wave %d rounds %d: %lld %lld %lld | %lld %lld %lld %lld | %lld %lld %lld %lld | %lld %lld %lld %lld %lld\n",
                   C, K, (int)BWD, (int)FOLD, (int)WG, (int)blockIdx.x, wv * 7, r_end - r_beg,
                   d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11], d[12], d[13], d[14], d[15]);
        }
    }
#endif
}

// One or two INDEPENDENT convolutions of the same template configuration in one launch (the up- / low-branch Bottleneck
// convolutions of an hourglass level): blocks [0, nblk[0]) work on descriptor 0, the rest on descriptor 1, spread evenly
// over the grid (pair_block, common.h).
struct C1Args { fpd_conv_t c[2]; int nblk[2]; };

template <int C, int K, bool BWD, bool FOLD, bool WG, bool RES, bool SKIP = false>
__global__ __launch_bounds__(512, 2) void c1_kernel(const C1Args p) {
    int isb, u;
    pair_block(blockIdx.x, gridDim.x, p.nblk[1], isb, u);
    c1_body<C, K, BWD, FOLD, WG, RES, SKIP>(p.c[isb], u, p.nblk[isb]);
}

// ---------------------------------------------------------------------------------------------------------------------
// FPD_C1: 0 = never, 1 = launches of >= FPD_C1_MIN_PX pixels (default), 2 = whenever the shape is in the domain (tests:
// fpd_set_option("conv_c1", v)); FPD_C1_BLOCKS: persistent blocks of a launch, default 192 of the 256 CUs
// (192, not 256: a resident block owns most of its CU's LDS, and the frozen teacher's fused Bottlenecks -- 128 blocks of 151 KB on
//  another stream -- need compute units of their own; r06 sweep inside the step, one box: 160 / 192 / 224 / 256 blocks ->
//  9.21 / 9.15 / 9.17-9.45 / 9.25 ms)
EnvOpt g_c1_mode{"FPD_C1", 1}, g_c1_blocks{"FPD_C1_BLOCKS", 192, 1};
// FPD_FUSE_SKIP (default 1; tests: fpd_set_option("conv_skip", v)): 0 = the second source (fpd_conv_t.x2) is not offered
EnvOpt g_c1_skip{"FPD_FUSE_SKIP", 1};
std::atomic<int> g_c1_launches{0};                       // launches this kernel has served (tests: "conv_c1_launches")
// Smallest launch (pixels) the kernel takes in mode 1, forward launches and data gradients apart.  Kernels alone on the small maps
// (profiles/r06_c1_small_maps.txt): the forward 128 -> 64 wins at every size (7.5 vs 8.9-9.2 us down to 4x4 = 512 pixels), the data
// gradients with their fused weight gradient lose 1 us to conv_tile's plain data gradient below 32x32 -- but take the weight gradient
// off the lane.  Inside the step (one box, three interleaved runs each): forward / backward 2048 / 2048 -> 8.763, 8.823, 8.764 ms;
// 512 / 2048 -> 8.762, 8.760, 8.747; 512 / 8192 -> 8.755, 8.750, 8.768; 512 / 16384 -> 8.796, 8.763, 8.807; the earlier sweep of
// both together: 32768 / 8192 / 2048 / 512 -> 9.669 / 9.60 / 9.574 / 9.581.
EnvOpt g_c1_min_px{"FPD_C1_MIN_PX", 512}, g_c1_min_px_bwd{"FPD_C1_MIN_PX_BWD", 2048};
int c1_fuse_wgrad() { return 1; }

bool c1_chan(int c) { return c == 32 || c == 64 || c == 128; }
bool c1_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// fold: decide for the launch as it will be made WITH a folded BN-backward apply, whatever a.fold_x holds now (ConvAsk); skip: WITH
// the second source the fields describe (forward C -> 2C, C in {32, 64}: K = 256 is outside c1_chan and stays two launches)
bool c1_domain(const fpd_conv_t& a, bool fold, bool skip = false) {
    if (skip) {
        if (g_c1_skip.get() == 0 || a.epi != FPD_EPI_PLAIN || a.residual != nullptr || a.x2 == nullptr || a.w2 == nullptr) return false;
        if (a.C2 != a.C || a.K != 2 * a.C || a.C > 64 || !c1_chan(a.C)) return false;
        if (!c1_aligned(a.x2) || !c1_aligned(a.w2) || a.y == a.x2) return false;
    }
    if (a.dtype != FPD_BF16 || a.R != 1 || a.S != 1 || a.stride != 1 || a.pad != 0 || a.P != a.H || a.Q != a.W) return false;
    // (16 -> 128: the inter-stack score_ convolution and the data gradient of the score convolution, hourglass.py:136-137, one k-step)
    if (!(c1_chan(a.C) || (a.C == 16 && a.K == 128)) || !c1_chan(a.K)) return false;
    const long long M = (long long)a.N * a.H * a.W;
    if (M % 32 != 0 || M > (1ll << 30)) return false;
    if (!c1_aligned(a.x) || !c1_aligned(a.y) || !c1_aligned(a.w) || !c1_aligned(a.residual) || !c1_aligned(a.epi_x) ||
        !c1_aligned(a.fold_x) || !c1_aligned(a.fold_out)) return false;
    if (a.epi == FPD_EPI_BNRELU_BWD) {
        // the data gradients of the hot path: no bias, no accumulate source, no prologue BN; dW tiles for every wave
        if (a.bias != nullptr || a.residual != nullptr || a.bn.mode != FPD_BN_NONE) return false;
        if (a.C == 16) { if (fold) return false; }                    // (no dW tiles: its weight gradient stays a separate launch)
        // 128 <-> 64 with the fused weight gradient; 128 x 128 (the dy + a(u) tiles of 8 waves do not fit the LDS) as a plain data
        // gradient, its weight gradient a launch of its own on the lane
        else if ((a.C / 32) * (a.K / 32) != C1_NW && !(a.C == 128 && a.K == 128 && !fold)) return false;
    } else {
        if (a.epi != FPD_EPI_PLAIN || a.y == a.x) return false;      // (a forward launch offers neither fusion: ConvRoute)
    }
    return true;
}
int c1_rounds(const fpd_conv_t& a) { return cdiv(a.N * a.H * a.W / 32, C1_NW); }

struct C1Plan { int na, nb, grid; bool wg; };
// The ONE decision of this unit, for the launch and for the queries: does the kernel take the launch (pair) carrying `ask`, with
// which grid, and which of the two fusions does it offer.  16 -> 128 and 128 x 128 data gradients are taken only unfolded (no FOLD
// variant: their folded launch goes on to the next kernel); the fused weight gradient needs a dW tile for every wave.
bool c1_route(const fpd_conv_t& a, const fpd_conv_t* b, ConvAsk ask, ConvRoute& r, C1Plan& pl) {
    const int mode = g_c1_mode.get();
    if (mode == 0 || !c1_domain(a, ask.fold, ask.skip) || (ask.skip && b != nullptr)) return false;
    const bool bwd = a.epi == FPD_EPI_BNRELU_BWD;
    long long px = (long long)a.N * a.H * a.W;
    if (b != nullptr) {
        if (!c1_domain(*b, ask.fold) || a.K != b->K || a.C != b->C || a.epi != b->epi) return false;
        if ((a.residual != nullptr) != (b->residual != nullptr)) return false;      // (the residual is a template parameter)
        px += (long long)b->N * b->H * b->W;
    }
    if (mode == 1 && px < (bwd ? g_c1_min_px_bwd : g_c1_min_px).get()) return false;
    if (!fpd_split_blocks(c1_rounds(a), b ? c1_rounds(*b) : 0, b != nullptr, g_c1_blocks.get(), pl.na, pl.nb)) return false;
    pl.grid = pl.na + pl.nb;
    pl.wg = ask.wg && c1_fuse_wgrad() != 0 && bwd && (a.C / 32) * (a.K / 32) == C1_NW;      // (a pair: same C, K, epilogue)
    r.folds = ask.fold && bwd;
    r.skips = ask.skip;
    r.slabs_a = pl.wg ? pl.na : 0;
    r.slabs_b = pl.wg ? pl.nb : 0;
    return true;
}

template <int C, int K, bool BWD, bool FOLD, bool WG, bool RES, bool SKIP = false>
int c1_launch_t(const fpd_conv_t& a, const fpd_conv_t* b, const C1Plan& pl, hipStream_t st) {
    static LdsAttr configured;
#ifdef FPD_C1_TIMING
    constexpr size_t lds = C1Geo<C, K, BWD, WG, SKIP>::LDS + 1024;
#else
    constexpr size_t lds = C1Geo<C, K, BWD, WG, SKIP>::LDS;
#endif
    static_assert(lds <= 160 * 1024, "conv_c1: LDS budget");
    if (int rc_ = configured.ensure(reinterpret_cast<const void*>(&c1_kernel<C, K, BWD, FOLD, WG, RES, SKIP>), lds)) return rc_;
    C1Args args;
    args.c[0] = a; args.c[1] = b ? *b : a; args.nblk[0] = pl.na; args.nblk[1] = pl.nb;
    FPD_LAUNCH((c1_kernel<C, K, BWD, FOLD, WG, RES, SKIP>), dim3(pl.grid), dim3(512), lds, st, args);
    g_c1_launches.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

template <int C, int K>
int c1_launch_ck(const fpd_conv_t& a, const fpd_conv_t* b, const C1Plan& pl, hipStream_t st) {
    if (a.epi == FPD_EPI_BNRELU_BWD) {
        if constexpr ((C / 32) * (K / 32) == C1_NW) {
            if (a.fold_x != nullptr || (b != nullptr && b->fold_x != nullptr))
                return pl.wg ? c1_launch_t<C, K, true, true, true, false>(a, b, pl, st) : c1_launch_t<C, K, true, true, false, false>(a, b, pl, st);
            return pl.wg ? c1_launch_t<C, K, true, false, true, false>(a, b, pl, st) : c1_launch_t<C, K, true, false, false, false>(a, b, pl, st);
        } else if constexpr (C == 16 || (C == 128 && K == 128)) {
            return c1_launch_t<C, K, true, false, false, false>(a, b, pl, st);
        } else {
            return 1;
        }
    }
    if (a.x2 != nullptr) {
        if constexpr (K == 2 * C && C >= 32 && C <= 64) return c1_launch_t<C, K, false, false, false, false, true>(a, nullptr, pl, st);
        else return 1;
    }
    if (a.residual != nullptr) return c1_launch_t<C, K, false, false, false, true>(a, b, pl, st);
    return c1_launch_t<C, K, false, false, false, false>(a, b, pl, st);
}

template <int C>
int c1_launch_c(const fpd_conv_t& a, const fpd_conv_t* b, const C1Plan& pl, hipStream_t st) {
    switch (a.K) {
        case 32: return c1_launch_ck<C, 32>(a, b, pl, st);
        case 64: return c1_launch_ck<C, 64>(a, b, pl, st);
        default: return c1_launch_ck<C, 128>(a, b, pl, st);
    }
}

}  // namespace

int fpd_conv_c1_option(int which, int value) {      // which: 0 = mode, 1 = blocks, 3 = second source offered (returns the previous value), 2 = launches served so far
    if (which == 2) return g_c1_launches.load(std::memory_order_relaxed);
    return (which == 3 ? g_c1_skip : which == 0 ? g_c1_mode : g_c1_blocks).set(value);
}

int fpd_conv_c1_route(const fpd_conv_t& a, const fpd_conv_t* b, ConvAsk ask, ConvRoute& r) {
    C1Plan pl;
    return c1_route(a, b, ask, r, pl) ? 0 : 1;
}
int fpd_conv_c1_launch(const fpd_conv_t& a, const fpd_conv_t* b, hipStream_t st) {
    ConvRoute r;
    C1Plan pl;
    if (!c1_route(a, b, fpd_conv_ask(a, b), r, pl)) return 1;
    if (int rc = fpd_conv_check_slabs(a, r.slabs_a, "conv_c1")) return rc;
    if (b != nullptr) {
        if (int rc = fpd_conv_check_slabs(*b, r.slabs_b, "conv_c1")) return rc;
        FPD_REQUIRE((a.wg_partial == nullptr) == (b->wg_partial == nullptr), "conv_pair: both or neither convolution of a pair take a fused weight gradient");
    }
    switch (a.C) {
        case 16: return c1_launch_ck<16, 128>(a, b, pl, st);
        case 32: return c1_launch_c<32>(a, b, pl, st);
        case 64: return c1_launch_c<64>(a, b, pl, st);
        default: return c1_launch_c<128>(a, b, pl, st);
    }
}
