// bneck_fused: one launch for a whole pre-activation Bottleneck of a FROZEN (eval-mode BN) hourglass:
//     y = x + conv3( relu(bn3( conv2( relu(bn2( conv1( relu(bn1(x)) ) )) ) )) )        (hourglass.py:32-52)
// with conv1 1x1 C->P, conv2 3x3 P->P (pad 1), conv3 1x1 P->C, C = 2P.  Eval-mode BN has no batch-wide dependency,
// so both P-channel intermediates stay in LDS: versus three conv launches this removes two tensor round trips through
// HBM (~45 % of the bytes at 64x64) and two of three launch latencies (all that matters at 4x4..16x16).
//
// One block = 128 consecutive output pixels (whole image rows, 128 % W == 0), 8 wave64, 1 block per CU.
//   phase A  conv1 over the tile PLUS its one-row halo (<= 2 passes of 128 pixels; K = C in chunks of 64 staged
//            through LDS with bn1+ReLU applied on the way in).  Result -> bn2+ReLU -> bf16 -> LDS image `a2`
//            laid out like conv_tile's halo tile (rows of W+2 pixels, explicit zero border columns, one zero pixel
//            that lanes whose tap row falls outside their image read instead).
//   phase B  conv2: 9 taps x K = P from `a2`; weight tiles [P][P] double-buffered in LDS, the next tile travelling
//            by LDS-DMA.  Result -> bn3+ReLU -> bf16 -> LDS `a3` (aliases a2).
//   phase C  conv3 = two more steps of the same pipeline (rows [0,P) and [P,2P) of w3 are [P][P] tiles), then the
//            epilogue: fp32 staging per wave, + bias + residual x, one rounding, 128-byte row segments to HBM.
// All MFMAs run "transposed" (first operand = weights, second = pixels): a lane then owns 4 CONSECUTIVE channels of
// one pixel per register quad, so the LDS intermediates are written as packed 8-byte vectors.
// Rounding: each intermediate is rounded to bf16 once (after bias+BN+ReLU); the 3-launch path rounds the raw conv
// output and again after BN.  oracle/plan_interp.py `run_bneck` is the specification of this op.
#include <algorithm>
#include <type_traits>

#include "conv_dispatch.h"
#include "fused_lds.h"
#include "fused_tile.h"

namespace {

// (register arrays are indexed through static_for: common.h)

#ifdef FPD_BNECK_TIMING          // probe build only (tools/bneck_bench.py): cycle stamps of block 0 at the phase boundaries
#define STAMP(i) do { if (tid == 0 && bid_in == 0) stamps[i] = clock64(); } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

// Folded per-channel tables, [3C + 4P] floats: sc1[C] sh1[C] | sc2[P] sh2'[P] | sc3[P] sh3'[P] | b3[C] with
// sh2' = sh2 + sc2*b1, sh3' = sh3 + sc3*b2 (conv biases folded into the following BN).
template <int P>
__device__ __forceinline__ void bneck_fold_tables(const fpd_bneck_t& a, float* out, int tid, int nthreads) {
    constexpr int C = 2 * P;
    for (int c = tid; c < C; c += nthreads) {
        float sc, sh;
        bn_coef_eval(a.bn1, c, sc, sh);
        out[c] = sc;
        out[C + c] = sh;
        out[2 * C + 4 * P + c] = a.b3 ? a.b3[c] : 0.f;
    }
    for (int c = tid; c < 2 * P; c += nthreads) {
        const bool second = c >= P;
        const int cc = second ? c - P : c;
        float sc, sh;
        bn_coef_eval(second ? a.bn3 : a.bn2, cc, sc, sh);
        const float* bias = second ? a.b2 : a.b1;
        out[2 * C + (second ? 2 * P : 0) + cc] = sc;
        out[2 * C + (second ? 2 * P : 0) + P + cc] = fmaf(sc, bias ? bias[cc] : 0.f, sh);
    }
}

template <int P>
__global__ void bneck_fold_kernel(const fpd_bneck_t a, float* out) { bneck_fold_tables<P>(a, out, threadIdx.x, blockDim.x); }

// Block bid_in of the nblk blocks assigned to fused Bottleneck `a`: persistent over its ntiles 128-pixel tiles
// (tile = bid_in, bid_in + nblk, ...).  A grid smaller than the CU count leaves compute units free for the
// latency-bound student kernels that run concurrently on another stream (a resident block owns its CU's LDS).
// The [P][P] weight tiles of phases B/C go HBM/L2 -> LDS by LDS-DMA (global_load_lds_dwordx4, no VGPR round trip, no
// ds_write pass): ring rows are unpadded (the DMA destination is lane-linear, 1 KiB per wave instruction) and bank
// conflicts are avoided by an XOR swizzle of the 16-byte chunks applied on the per-lane SOURCE address and again on
// the fragment reads (chunk c of row r sits at position c ^ sw(r)).  (The register path of round 1 is gone: it was never faster,
// and its P = 64 variant spilled in the tap loop.)
// UPADD: x is not a tensor but the sum the hourglass forms in front of this Bottleneck, x[p] = round_bf16(up1[p] + low[p / 2])
// (hourglass.py:80-92) with up1 = a.x and low = a.x2 at half resolution.  Both places that read x -- the phase-A staging and the
// residual rows of the epilogue -- load the two sources and round their fp32 sum to bf16 once, which is bit for bit what the
// stand-alone FPD_EW_UPADD_FWD launch stored: the 2 x [N,H,W,C] round trip of that tensor through HBM is gone.  The low pixel of
// global image row g (= n*H + row; H and n*H are even), column j is row g >> 1, column j >> 1 of the [N*H/2][W/2] grid.
template <int P, bool UPADD>
__device__ __forceinline__ void bneck_eval_body(const fpd_bneck_t& a, const int logW, const int bid_in, const int nblk, const int ntiles) {
    using L = BneckLds<P>;                      // the LDS layout (fused_lds.h): tables | a2 image | R2
    constexpr int C = L::C, LDX = L::LDX, LD2 = L::LD2, CW = L::CW, ASTG = L::ASTG;
    constexpr int TNH = P / 64;                 // 32-channel MFMA tiles per wave (a wave owns half of a P-wide tile)
    constexpr int NSTEP = 9 + 2;
    constexpr int W1V = P * 8 / 512;            // vectors per thread of a [P][64] w1 chunk
    constexpr int NCH = C / 64;                 // channel chunks of conv1's reduction (even)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef FPD_BNECK_TIMING
    long long stamps[8];
    long long astamp[10];                        // phase A: [0] before the first staging, then after every chunk step
    int acnt = 0;
#define ASTAMP() do { if (tid == 0 && bid_in == 0 && acnt < 10) astamp[acnt++] = clock64(); } while (0)
#else
#define ASTAMP() do { } while (0)
#endif
    STAMP(0);
    const int q = wave & 3, hC = wave >> 2;     // pixel group (32 px) and channel half of this wave
    const int koff = 8 * (lane >> 5);
    const int H = a.H, W = a.W;
    const int M = a.N * H * W, GR = a.N * H;
    const int nrows = 128 >> logW, hrows = nrows + 2, WP = W + 2;
    // The a2 image is a RING of 2*nrows rows (two half-slots of nrows rows): halo row hr of tile T is "virtual row"
    // T*nrows + hr and lives in ring row (T*nrows + hr) mod 2*nrows.  Consecutive tiles of one image share two halo rows and the
    // ring keeps what the previous tile computed: tile T+1 only runs conv1 over its nrows NEW rows (one 128-pixel pass instead
    // of two: phase A was 40 % of a tile at 2x recompute, r02 stamps), and a3 of tile T goes into T's first half-slot, which
    // is dead by then (nrows * (W + 2) >= 128 pixels).
    const int rrows = 2 * nrows;
    const bool whole = L::whole(H, W);                   // tiles made of whole images keep the plain layout (no halo rows are read)
    const int irows = L::irows(whole, nrows);            // rows of the a2 image
    const int zero_px = irows * WP;
    int m0 = 0, g0 = 0;                          // first pixel / first image row of the current tile
    int vrow0 = 0;                               // virtual row of halo row 0 of the current tile, mod 2*nrows

    float* s_sc1 = reinterpret_cast<float*>(smem);
    float* s_sh1 = s_sc1 + C;
    float* s_sc2 = s_sh1 + C;
    float* s_sh2 = s_sc2 + P;
    float* s_sc3 = s_sh2 + P;
    float* s_sh3 = s_sc3 + P;
    float* s_b3 = s_sh3 + P;
    bf16_t* sA2 = reinterpret_cast<bf16_t*>(s_sc1 + L::TAB);
    bf16_t* sR2 = sA2 + L::image_px(irows, W) * LD2;     // (the 3 zero pixels sit at zero_px)
    const bf16_t* __restrict__ x = reinterpret_cast<const bf16_t*>(a.x);
    const bf16_t* __restrict__ x2 = reinterpret_cast<const bf16_t*>(UPADD ? a.x2 : nullptr);
    const bf16_t* __restrict__ w1 = reinterpret_cast<const bf16_t*>(a.w1);
    const bf16_t* __restrict__ w2 = reinterpret_cast<const bf16_t*>(a.w2);
    const bf16_t* __restrict__ w3 = reinterpret_cast<const bf16_t*>(a.w3);

    // ---- phase-A addressing (hoisted: the pipeline steps below must not spend VALU cycles on address arithmetic) ----
    // Tiles made of whole images never read their halo rows (every out-of-image tap is redirected to the zero pixels):
    // one pass over the tile's own 128 pixels (halo-pixel index W..W+127) is enough.
    int hp0 = whole ? W : 0;                             // per tile (below): 2 W when the first two halo rows are in the ring already
    int npass = whole ? 1 : ((hrows * W + 127) >> 7);
    const int xpx = tid >> 3, xcv = (tid & 7) * 8;       // this thread stages pixels xpx, xpx+64, channels xcv..+7
    int xo[2];                                           // element offsets of the two pixels in the pass being loaded
    int xo2[UPADD ? 2 : 1];                              // UPADD: the same for their low-branch pixels
    bool xok[2];
    auto pass_addr = [&](int p) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int hp = hp0 + 128 * p + xpx + 64 * i;
            const int hr = hp >> logW, j = hp & (W - 1);
            const int g = g0 - 1 + hr;
            xok[i] = hr < hrows && (unsigned)g < (unsigned)GR;
            xo[i] = xok[i] ? (g * W + j) * C + xcv : 0;
            if constexpr (UPADD) xo2[i] = xok[i] ? ((((g >> 1) << logW) >> 1) + (j >> 1)) * C + xcv : 0;
        }
    };
    int w1o[W1V], w1l[W1V];
#pragma unroll
    for (int i = 0; i < W1V; ++i) {
        const int v = tid + i * 512;
        w1o[i] = (v >> 3) * C + (v & 7) * 8;
        w1l[i] = 128 * LDX + (v >> 3) * LDX + (v & 7) * 8;
    }
    const int xl = xpx * LDX + xcv;

    u32x4 rx[NCH][2], rw[NCH][W1V];
    u32x4 rx2[UPADD ? NCH : 1][2];
    auto a_load = [&](auto kcc) __attribute__((always_inline)) {
        constexpr int kc = decltype(kcc)::value;
        static_for<2>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const u32x4 z = {0u, 0u, 0u, 0u};
            rx[kc][i] = z;
            if (xok[i]) rx[kc][i] = *reinterpret_cast<const u32x4*>(x + (xo[i] + kc * 64));
            if constexpr (UPADD) {
                rx2[kc][i] = z;
                if (xok[i]) rx2[kc][i] = *reinterpret_cast<const u32x4*>(x2 + (xo2[i] + kc * 64));
            }
        });
        static_for<W1V>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            rw[kc][i] = *reinterpret_cast<const u32x4*>(w1 + (w1o[i] + kc * 64));
        });
    };
    // UPADD: vector i of slot kc becomes x = round(up1 + low), as the up-add launch stored it; a_store_slice then stages rx as
    // it always did.  The sums are VALU work like the staging and ride behind the MFMAs of the chunk steps in the same way (below).
    auto a_sum = [&](auto kcc, auto ic) __attribute__((always_inline)) {
        constexpr int kc = decltype(kcc)::value, i = decltype(ic)::value;
        if constexpr (UPADD) rx[kc][i] = bf16x8_sum(rx[kc][i], rx2[kc][i]);
    };
    // staging of chunk kc in NSL = 2 + W1V slices (x vector 0, x vector 1, then the w1 vectors): the chunk loop places one
    // slice behind the MFMAs of each k-step, so that the VALU / LDS-store work of the next chunk runs while the matrix
    // pipe executes (a wave issues in order: staged as one block it would only start once all MFMAs of the step are issued)
    constexpr int NSL = 2 + W1V;
    auto a_store_slice = [&](auto kcc, auto slc) __attribute__((always_inline)) {
        constexpr int kc = decltype(kcc)::value, sl = decltype(slc)::value;
        bf16_t* dst = sR2 + (kc & 1) * ASTG;
        if constexpr (sl < 2) {
            f32x4 sc[2], sh[2];
            sc[0] = *reinterpret_cast<const f32x4*>(s_sc1 + kc * 64 + xcv);
            sc[1] = *reinterpret_cast<const f32x4*>(s_sc1 + kc * 64 + xcv + 4);
            sh[0] = *reinterpret_cast<const f32x4*>(s_sh1 + kc * 64 + xcv);
            sh[1] = *reinterpret_cast<const f32x4*>(s_sh1 + kc * 64 + xcv + 4);
            float f[8];
            const u32x4 r = rx[kc][sl];
            DT<bf16_t>::unpack(make_uint4(r[0], r[1], r[2], r[3]), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = fmaxf(fmaf(f[e], sc[e >> 2][e & 3], sh[e >> 2][e & 3]), 0.f);
            *reinterpret_cast<uint4*>(dst + xl + 64 * sl * LDX) = DT<bf16_t>::pack(f);
        } else if constexpr (sl < NSL) {
            *reinterpret_cast<u32x4*>(dst + w1l[sl - 2]) = rw[kc][sl - 2];
        }
    };
    auto a_store = [&](auto kcc) __attribute__((always_inline)) {
        static_for<NSL>([&](auto slc) { a_store_slice(kcc, slc); });
    };
    // ---- weight-tile pipeline of phases B/C: tile s is requested one step before the step that multiplies with it ----
    // LDS-DMA of weight tile s into ring buffer s & 1: P rows of 2P bytes = P*P*2/1024 wave instructions, 8 waves.
    // Wave instruction q covers ring bytes [q*1024, q*1024 + 1024): rows q*RPI .. +RPI, lane L -> row q*RPI + L/CPR,
    // position L % CPR, fetching global chunk (position ^ sw(row)) of that row.
    constexpr int CPR = P / 8;                  // 16-byte chunks per weight row
    constexpr int RPI = 64 / CPR;               // rows per wave instruction
    constexpr int DPW = P / RPI / 8;            // wave instructions per wave per tile
    // per-lane byte offsets of the DPW pieces this wave fetches of a tile, for the w2 ([P][9][P]) and w3 ([C][P]) row pitches;
    // the step's constant part (s*P resp. (s-9)*P*P elements) is added at issue time
    unsigned dma2[DPW], dma3[DPW];
#pragma unroll
    for (int j = 0; j < DPW; ++j) {
        const int row = wave * DPW * RPI + j * RPI + lane / CPR;
        const int sw = (P == 128) ? (row & 15) : ((row >> 1) & 7);      // sw(row): 16 consecutive rows -> 16 slots
        const int c8 = ((lane % CPR) ^ sw) * 8;
        dma2[j] = (unsigned)(row * 9 * P + c8) * 2u;
        dma3[j] = (unsigned)(row * P + c8) * 2u;
    }
    auto t_dma = [&](auto sc_) __attribute__((always_inline)) {
        constexpr int s = decltype(sc_)::value;
        unsigned char* ring = reinterpret_cast<unsigned char*>(sR2) + (s & 1) * L::RING * 2 + wave * DPW * 1024;
        const char* gbase = s < 9 ? reinterpret_cast<const char*>(w2) + s * P * 2
                                  : reinterpret_cast<const char*>(w3) + (s - 9) * P * P * 2;
        static_for<DPW>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            unsigned off = s < 9 ? dma2[j] : dma3[j];
            asm volatile("" : "+v"(off));    // keep the 44 (step, piece) addresses from being hoisted out of the tile loop
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + off),
                                             (__attribute__((address_space(3))) void*)(ring + j * 1024), 16, 0, 0);
        });
    };

    // ---- tables (once per block): folded by the host-side prep pass (a.folded) or here ----
    if (a.folded != nullptr) {
        for (int v = tid; v < L::TAB / 4; v += 512)
            reinterpret_cast<f32x4*>(s_sc1)[v] = reinterpret_cast<const f32x4*>(a.folded)[v];
    } else {
        bneck_fold_tables<P>(a, s_sc1, tid, 512);
    }

    // a block owns a CONTIGUOUS range of tiles (consecutive row groups of an image), so that the ring pays off
    const int t_beg = fpd_cut(bid_in, ntiles, nblk), t_end = fpd_cut(bid_in + 1, ntiles, nblk);
    for (int tile = t_beg; tile < t_end; ++tile) {
    {
        m0 = tile * 128;
        g0 = m0 >> logW;
        vrow0 = (tile * nrows) % rrows;
        if (!whole) {
            // halo rows 0 and 1 (= the previous tile's last two rows) are cached unless this is the block's first tile or the
            // tile starts a new image (then row 0 is outside the image and never read.  Row 1 IS in the ring even then: conv1 is
            // pointwise and the previous tile filled its last halo row from the tensor whatever image the row belongs to, so
            // dropping the second term changes no output bit -- tests/test_teacher_persistent_gpu.py pass either way; it
            // is kept because an image's first tile then depends on nothing the previous image left behind)
            const bool incr = tile > t_beg && (g0 % H) != 0;
            hp0 = incr ? 2 * W : 0;
            npass = incr ? 1 : ((hrows * W + 127) >> 7);
        }
    }
    // first loads of the tile go out before anything else
    pass_addr(0);
    static_for<NCH>([&](auto kcc) { a_load(kcc); });
    if (npass > 1) pass_addr(1);
    __syncthreads();                             // tables visible; previous tile's epilogue is done with the LDS
    // zero border columns of every halo row + the zero pixels (whole LD2 rows, 16-byte vectors); per tile, because
    // the a3 image of the previous tile overwrote the first 128 rows
    {
        constexpr int VR = LD2 / 8;
        const uint4 z = make_uint4(0, 0, 0, 0);
        for (int v = tid; v < (2 * irows + 3) * VR; v += 512) {
            const int pz = v / VR, cv = (v - pz * VR) * 8;
            const int px = pz < 2 * irows ? ((pz >> 1) * WP + ((pz & 1) ? WP - 1 : 0)) : zero_px + (pz - 2 * irows);
            *reinterpret_cast<uint4*>(sA2 + px * LD2 + cv) = z;
        }
    }
    // (UPADD) chunk 0 of the tile's first loads is staged right below: summed here.  Chunks 1.. follow in the chunk steps.
    a_sum(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    a_sum(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
    STAMP(1);

    // =========================== phase A: conv1 over the halo rows ===========================
    // All NCH channel chunks of a pass are in flight in registers; the slot a chunk frees is refilled with the same
    // chunk of the NEXT pass.  Staging is double-buffered: chunk k+1 gets its bn1+ReLU and goes to LDS while the MFMAs
    // of chunk k run; one barrier per chunk.
    auto refill = [&](auto kcc, int pp) __attribute__((always_inline)) {      // slot kcc held pass pp, now stored
        if (pp + 1 < npass) a_load(kcc);                                       // xo/xok already describe pass pp+1
    };
#ifdef FPD_BNECK_TIMING
    acnt = 0;
#endif
    ASTAMP();
    a_store(std::integral_constant<int, 0>{});
    refill(std::integral_constant<int, 0>{}, 0);
    __syncthreads();
    ASTAMP();
    for (int p = 0; p < npass; ++p) {
        f32x16 acc[TNH];
#pragma unroll
        for (int tn = 0; tn < TNH; ++tn)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[tn][i] = 0.f;
        static_for<NCH>([&](auto kcc) {
            constexpr int kc = decltype(kcc)::value;
            // slice sl of the staging of the NEXT chunk (next pass's chunk 0 behind the last chunk) + the refill of its slot
            auto stage_slice = [&](auto slc, auto lastc) __attribute__((always_inline)) {
                constexpr bool last = decltype(lastc)::value;
                if constexpr (kc + 1 < NCH) {
                    a_store_slice(std::integral_constant<int, (kc + 1) % NCH>{}, slc);
                    if constexpr (last) refill(std::integral_constant<int, (kc + 1) % NCH>{}, p);
                } else {
                    if (p + 1 < npass) {
                        a_store_slice(std::integral_constant<int, 0>{}, slc);
                        if constexpr (last) {
                            if (p + 2 < npass) pass_addr(p + 2);               // (never taken: npass <= 2)
                            refill(std::integral_constant<int, 0>{}, p + 1);
                        }
                    }
                }
            };
            const bf16_t* xrow = sR2 + (kc & 1) * ASTG + (q * 32 + (lane & 31)) * LDX + koff;
            const bf16_t* wrow = sR2 + (kc & 1) * ASTG + 128 * LDX + (hC * CW + (lane & 31)) * LDX + koff;
            static_for<4>([&](auto kkc) {
                constexpr int kk = decltype(kkc)::value;
                const bf16x8 px = *reinterpret_cast<const bf16x8*>(xrow + kk * 16);
#pragma unroll
                for (int tn = 0; tn < TNH; ++tn) {
                    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wrow + tn * 32 * LDX + kk * 16);
                    acc[tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, px, acc[tn], 0, 0, 0);
                }
                if constexpr (!UPADD) {
                    stage_slice(kkc, std::integral_constant<bool, kk == NSL - 1>{});      // NSL <= 4 slices, one per k-step
                } else {
                    // the x vectors of the next chunk are summed behind k-steps 0 and 1 and staged behind 2 and 3, the w1 vectors
                    // go first.  Slots of the tile's first loads are summed here, just before their staging (pass 0, chunks 1..);
                    // a slot refilled for the next pass is summed one step after its request (the barrier has drained it): slot
                    // kc behind k-steps 2 and 3 of this step.
                    if constexpr (kk < 2) {
                        if constexpr (kc + 1 < NCH) {
                            if (p == 0) a_sum(std::integral_constant<int, (kc + 1) % NCH>{}, kkc);
                        }
                        stage_slice(std::integral_constant<int, (kk + 2 < NSL ? kk + 2 : NSL)>{}, std::false_type{});
                    } else {
                        stage_slice(std::integral_constant<int, kk - 2>{}, std::integral_constant<bool, kk == 3>{});
                        if (p + 1 < npass) a_sum(kcc, std::integral_constant<int, kk - 2>{});
                    }
                }
            });
            __syncthreads();
            ASTAMP();
        });
        if (p + 1 == npass) {                    // both staging buffers are dead: the first two weight tiles of phase B
            t_dma(std::integral_constant<int, 0>{});     // travel while the a2 image is written out
            t_dma(std::integral_constant<int, 1>{});
        }
        // a2 = relu(bn2(conv1 + b1)) as bf16; rows of the zero-column layout.  Halo pixels outside the tensor hold
        // junk that no lane reads (their readers are redirected to the zero pixels).
        const int hp = hp0 + 128 * p + q * 32 + (lane & 31);
        const int hr = hp >> logW, j = hp & (W - 1);
        if (hr < hrows) {
            const int rr = whole ? hr : ((vrow0 + hr) & (rrows - 1));
            act_store(acc, s_sc2, s_sh2, hC * CW, lane, sA2 + (rr * WP + j + 1) * LD2);
        }
    }

    // =========================== phases B + C: 11-step weight-tile pipeline ===========================
    const int ml = q * 32 + (lane & 31);
    const int a3px = whole ? 0 : vrow0 * WP;     // a3 overwrites this tile's first half-slot (its rows are dead after conv2)
    int ab[3];
    {
        const int ti = ml >> logW, tj = ml & (W - 1);
        const int g = g0 + ti;
        const int pr = g % H;
        const bool live = g < GR;
        const int r0 = whole ? ti : ((vrow0 + ti) & (rrows - 1)), r1 = whole ? ti + 1 : ((vrow0 + ti + 1) & (rrows - 1)),
                  r2 = whole ? ti + 2 : ((vrow0 + ti + 2) & (rrows - 1));
        ab[0] = (live && pr - 1 >= 0) ? (r0 * WP + tj) * LD2 : zero_px * LD2;
        ab[1] = live ? (r1 * WP + tj) * LD2 : zero_px * LD2;
        ab[2] = (live && pr + 1 < H) ? (r2 * WP + tj) * LD2 : zero_px * LD2;
    }
    STAMP(2);
    __syncthreads();                             // tiles 0 and 1 + the whole a2 image visible
    STAMP(3);

    f32x16 accB[TNH], accC[2][TNH];
#pragma unroll
    for (int tn = 0; tn < TNH; ++tn)
#pragma unroll
        for (int i = 0; i < 16; ++i) accB[tn][i] = 0.f;

    const int wsw = (P == 128) ? (lane & 15) : ((lane >> 1) & 7);     // sw(row) of this lane's weight rows
    // one pipeline step: K = P from pixel row `arow` against weight tile `buf`; behind(kkc) is issued behind the MFMAs of k-step kk
    auto mma = [&](const bf16_t* arow, int buf, f32x16* acc, auto behind) __attribute__((always_inline)) {
        const bf16_t* wbase = sR2 + buf * L::RING + (hC * CW + (lane & 31)) * P;
        static_for<P / 16>([&](auto kkc) {
            constexpr int kk = decltype(kkc)::value;
            const bf16x8 px = *reinterpret_cast<const bf16x8*>(arow + kk * 16);
            const int wo = ((2 * kk + (lane >> 5)) ^ wsw) * 8;
#pragma unroll
            for (int tn = 0; tn < TNH; ++tn) {
                const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wbase + tn * 32 * P + wo);
                acc[tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, px, acc[tn], 0, 0, 0);
            }
            behind(kkc);
        });
    };

    // residual rows of the epilogue, requested under the last pipeline steps (the kernel's own text, like the head's: fused_tile.h)
    constexpr int VW = CW / 8;                   // output vectors per pixel row of this wave's channel slice
    constexpr int NIT = 32 * VW / 64;
    u32x4 rres[2][NIT];
    u32x4 rres2[UPADD ? NIT : 1];                // UPADD: the low-branch vectors of the rows requested last, until res_sum folds them in
    auto res_load = [&](auto stc) __attribute__((always_inline)) {
        constexpr int st = decltype(stc)::value;
        static_for<NIT>([&](auto itc) {
            constexpr int it = decltype(itc)::value;
            const int idx = lane + 64 * it;
            const int px = idx / VW, cv = (idx - px * VW) * 8;
            const int m = m0 + q * 32 + px;
            const u32x4 z = {0u, 0u, 0u, 0u};
            rres[st][it] = z;
            if (m < M) rres[st][it] = *reinterpret_cast<const u32x4*>(x + ((size_t)m * C + st * P + hC * CW + cv));
            if constexpr (UPADD) {
                const int g = m >> logW, j = m & (W - 1);
                const int m2 = (((g >> 1) << logW) >> 1) + (j >> 1);
                rres2[it] = z;
                if (m < M) rres2[it] = *reinterpret_cast<const u32x4*>(x2 + ((size_t)m2 * C + st * P + hC * CW + cv));
            }
        });
    };
    // UPADD: the residual is the same rounded sum that phase A staged.  Formed one pipeline step after the request (the barrier
    // in between has drained the loads), one vector behind the MFMAs of each of the first NIT k-steps of steps 9 and 10; the
    // epilogue then reads rres as it always did.
    auto res_sum = [&](auto stc, auto itc) __attribute__((always_inline)) {
        constexpr int st = decltype(stc)::value, it = decltype(itc)::value;
        if constexpr (UPADD && it < NIT) rres[st][it] = bf16x8_sum(rres[st][it], rres2[it]);
    };

    static_for<NSTEP>([&](auto sc_) {
        constexpr int s = decltype(sc_)::value;
        // tile s+1 goes into the buffer tile s-1 left (every wave is past step s-1's barrier); tiles 0/1 were issued
        // at the end of phase A.  The barrier closing this step drains it (hipcc emits vmcnt(0) in front of s_barrier).
        if constexpr (s >= 1 && s + 1 < NSTEP) t_dma(std::integral_constant<int, (s + 1 < NSTEP ? s + 1 : 0)>{});
        if constexpr (s < 9) {
            mma(sA2 + ab[s / 3] + (s % 3) * LD2 + koff, s & 1, accB, [](auto) {});
        } else {
#pragma unroll
            for (int tn = 0; tn < TNH; ++tn)
#pragma unroll
                for (int i = 0; i < 16; ++i) accC[s - 9][tn][i] = 0.f;
            mma(sA2 + (a3px + ml) * LD2 + koff, s & 1, accC[s - 9],       // a3 aliases the dead half of a2: [128 px][LD2]
                [&](auto kkc) { res_sum(std::integral_constant<int, s - 9>{}, kkc); });
        }
        if constexpr (s + 1 < NSTEP) {
            if constexpr (s == 8) res_load(std::integral_constant<int, 0>{});
            if constexpr (s == 9) res_load(std::integral_constant<int, 1>{});
            __syncthreads();
        }
        if constexpr (s == 8) {
            STAMP(4);
            // every wave is past its last a2 read: a3 = relu(bn3(conv2 + b2)) overwrites the image
            act_store(accB, s_sc3, s_sh3, hC * CW, lane, sA2 + (a3px + ml) * LD2);
            __syncthreads();
        }
    });

    STAMP(5);
    // =========================== epilogue: y = conv3 + b3 + x ===========================
    float* stage = reinterpret_cast<float*>(sR2) + wave * 32 * L::LST;     // wave-private [32 px][CW + 4] fp32
    bf16_t* __restrict__ y = reinterpret_cast<bf16_t*>(a.y);
    static_for<2>([&](auto stc) {
        constexpr int st = decltype(stc)::value;
        __syncthreads();                         // weight tiles consumed / previous staging read back
        epi_stage<TNH>(accC[st], stage, lane);
        __syncthreads();
        static_for<NIT>([&](auto itc) {
            constexpr int it = decltype(itc)::value;
            const int idx = lane + 64 * it;
            const int px = idx / VW, cv = (idx - px * VW) * 8;
            const int m = m0 + q * 32 + px;
            if (m < M) {
                const int c = st * P + hC * CW + cv;
                *reinterpret_cast<uint4*>(y + ((size_t)m * C + c)) = epi_vec(stage + px * L::LST + cv, s_b3 + c, rres[st][it]);
            }
        });
    });
    }   // tile loop
#ifdef FPD_BNECK_TIMING
    STAMP(6);
    if (tid == 0 && bid_in == 0)
        printf("bneck W=%d: setup %lld | phaseA %lld | tile0 %lld | B(9 taps) %lld | a3+C %lld | epilogue %lld | total %lld cycles\n",
               W, stamps[1] - stamps[0], stamps[2] - stamps[1], stamps[3] - stamps[2], stamps[4] - stamps[3],
               stamps[5] - stamps[4], stamps[6] - stamps[5], stamps[6] - stamps[0]);
    if (tid == 0 && bid_in == 0 && acnt == 10)
        printf("  phase A steps: first-stage %lld | pass0 %lld %lld %lld %lld | pass1 %lld %lld %lld %lld | a2 write %lld\n",
               astamp[1] - astamp[0], astamp[2] - astamp[1], astamp[3] - astamp[2], astamp[4] - astamp[3], astamp[5] - astamp[4],
               astamp[6] - astamp[5], astamp[7] - astamp[6], astamp[8] - astamp[7], astamp[9] - astamp[8], stamps[2] - astamp[9]);
#endif
}

template <int P, bool UPADD>
__global__ __launch_bounds__(512, 1) void bneck_eval_kernel(const fpd_bneck_t a, const int logW, const int ntiles) {
    bneck_eval_body<P, UPADD>(a, logW, blockIdx.x, gridDim.x, ntiles);
}

// Two independent fused Bottlenecks (the up-branch and the low-branch one of an hourglass level) in one launch.
template <int P>
__global__ __launch_bounds__(512, 1) void bneck_eval_pair_kernel(const fpd_bneck_t a, const fpd_bneck_t b, const int logWa,
                                                                 const int logWb, const int nblk_a, const int ntiles_a,
                                                                 const int ntiles_b) {
    if ((int)blockIdx.x < nblk_a) bneck_eval_body<P, false>(a, logWa, blockIdx.x, nblk_a, ntiles_a);
    else bneck_eval_body<P, false>(b, logWb, (int)blockIdx.x - nblk_a, (int)gridDim.x - nblk_a, ntiles_b);
}

// grid cap of the persistent kernel (FPD_BNECK_BLOCKS): below the CU count so that concurrently running streams find free compute units.
// Measured (r01, pipelined step): 1024/256/224/192/160/128 -> 13.56/13.86/13.37/13.30/13.21/13.23 ms;
// r02 (wgrad batches of 8, same box): 96/112/128/144/160 -> 11.71/11.69/11.51/11.68/11.67 ms
static GridCap g_bneck_cap{"FPD_BNECK_BLOCKS", 128};

template <int P>
int launch_bneck_pair(const fpd_bneck_t& a, const fpd_bneck_t& b, hipStream_t st) {
    const size_t lds = std::max(BneckLds<P>::bytes(a.H, a.W), BneckLds<P>::bytes(b.H, b.W));
    static LdsAttr configured;        // per device, set once (thread-safe: common.h)
    if (int rc_ = configured.ensure(reinterpret_cast<const void*>(&bneck_eval_pair_kernel<P>), lds)) return rc_;
    int la = 0, lb = 0;
    while ((1 << la) < a.W) ++la;
    while ((1 << lb) < b.W) ++lb;
    const int ta = cdiv(a.N * a.H * a.W, 128), tb = cdiv(b.N * b.H * b.W, 128);
    int na = ta, nb = tb;
    const int cap = g_bneck_cap.get();
    if (ta + tb > cap) {                       // persistent: split the capped grid in proportion to the work
        const int capb = std::max(1, (int)((int64_t)cap * tb / (ta + tb)));
        nb = fpd_balanced_blocks(tb, capb);
        na = fpd_balanced_blocks(ta, std::max(1, cap - nb));
    }
    FPD_LAUNCH((bneck_eval_pair_kernel<P>), dim3(na + nb), dim3(512), lds, st, a, b, la, lb, na, ta, tb);
    return 0;
}

template <int P, bool UPADD>
int launch_bneck(const fpd_bneck_t& a, int logW, hipStream_t st) {
    const size_t lds = BneckLds<P>::bytes(a.H, a.W);
    static LdsAttr configured;        // per device, set once (thread-safe: common.h)
    if (int rc_ = configured.ensure(reinterpret_cast<const void*>(&bneck_eval_kernel<P, UPADD>), lds)) return rc_;
    const int ntiles = cdiv(a.N * a.H * a.W, 128);
    FPD_LAUNCH((bneck_eval_kernel<P, UPADD>), dim3(fpd_balanced_blocks(ntiles, g_bneck_cap.get())), dim3(512), lds, st, a, logW, ntiles);
    return 0;
}

}  // namespace

// fpd_set_option("bneck_blocks", n): the grid cap, any n >= 1 (tests: one block then walks many tiles of a small tensor);
// returns the previous value
int fpd_bneck_blocks_option(int value) { return g_bneck_cap.set(value); }

static bool bneck_in_domain(const fpd_bneck_t& a) {
    if (a.dtype != FPD_BF16 || a.C != 2 * a.P || (a.P != 64 && a.P != 128)) return false;
    if (a.W < 4 || a.W > 64 || (a.W & (a.W - 1)) != 0) return false;
    const int hw = a.H * a.W;
    return hw % 128 == 0 || 128 % hw == 0;                    // a tile is whole rows of one image, or whole images
}

// ---- up-add on load (fpd_bneck_t.x2) ----
static EnvOpt g_bneck_upadd{"FPD_BNECK_UPADD", 1};
int fpd_bneck_upadd_option(int value) { return g_bneck_upadd.set(value < 0 ? 0 : value); }

// nullptr = a launch of these dimensions with a low-branch source is served, else the reason.  Dimensions, dtype and the option
// only: the lowering asks before memory is planned.  (Up-add results are never 4 wide: their low branch is at least 4 x 4.)
const char* fpd_bneck_upadd_why_not(const fpd_bneck_t& a) {
    if (g_bneck_upadd.get() == 0) return "switched off (FPD_BNECK_UPADD=0 / option bneck_upadd)";
    if (!bneck_in_domain(a)) return "the shape is outside the fused kernel's domain";
    if (a.W < 8) return "W must be one of 8, 16, 32, 64";
    if (a.H & 1) return "H must be even";
    return nullptr;
}

// 0 = launched, 1 = shape outside this kernel's domain, <0 = error
int fpd_bneck_fused_launch(const fpd_bneck_t& a, hipStream_t st) {
    if (!bneck_in_domain(a)) return 1;
    int logW = 0;
    while ((1 << logW) < a.W) ++logW;
    if (a.x2 != nullptr) {
        if (fpd_bneck_upadd_why_not(a) != nullptr) return 1;      // (api.hip refused it with the reason already)
        return a.P == 128 ? launch_bneck<128, true>(a, logW, st) : launch_bneck<64, true>(a, logW, st);
    }
    return a.P == 128 ? launch_bneck<128, false>(a, logW, st) : launch_bneck<64, false>(a, logW, st);
}

// 0 = both launched as one kernel, 1 = not pairable (caller launches them one by one)
int fpd_bneck_fused_pair_launch(const fpd_bneck_t& a, const fpd_bneck_t& b, hipStream_t st) {
    if (!bneck_in_domain(a) || !bneck_in_domain(b) || a.P != b.P || a.x2 != nullptr || b.x2 != nullptr) return 1;
    return a.P == 128 ? launch_bneck_pair<128>(a, b, st) : launch_bneck_pair<64>(a, b, st);
}

// folded tables ([3C + 4P] floats) for a.folded; 1 = P not supported
int fpd_bneck_fold_launch(const fpd_bneck_t& a, float* out, hipStream_t st) {
    if (a.C != 2 * a.P || (a.P != 64 && a.P != 128)) return 1;
    if (a.P == 128) FPD_LAUNCH((bneck_fold_kernel<128>), dim3(1), dim3(256), 0, st, a, out);
    else FPD_LAUNCH((bneck_fold_kernel<64>), dim3(1), dim3(256), 0, st, a, out);
    return 0;
}
