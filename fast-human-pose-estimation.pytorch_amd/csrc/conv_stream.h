// Device pieces shared by the streaming convolution kernels (conv_c1, conv_c3; conv_pp takes the first two): packed
// bf16-pair arithmetic, the coefficients of a folded BN-backward apply, the table prologue in two halves, the per-channel
// epilogue arithmetic on one 16-byte vector and the one-per-block statistics flush.  Everything here is __forceinline__ and
// written so that it compiles to what the kernels held as their own text (profiles/convstream_isa.txt):
// the loops, the tile addressing and the stores stay in the kernels.
#pragma once
#include "common.h"

// Two bf16 of a dword as two floats and back: the forward arithmetic of the kernels is written on PAIRS (v_pk_fma_f32 / v_pk_add_f32 /
// v_pk_mul_f32, v_pk_max_i16 on the packed result) -- the same operation per element in the same order as the scalar form, so the
// same bits, at fewer vector instructions (r04 ISA count of conv_pp's 1x1 128->64 forward tile loop: 513 -> 406 per tile and wave,
// against 8 MFMAs).  Measured (r04, interleaved A/B + per-shape trace A/B): 2-4 % on the 1x1 forward launches in isolation, nothing
// on the step -- that tile loop is bound by its barriers and LDS round trips, not by VALU issue.  conv_pp's BN-backward epilogue stays
// scalar: its packed form was 2-7 % slower on the +wgrad +fold kernels (more registers, longer dependent chains).
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 bf2_unpack(unsigned w) {
    f32x2 r = {__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
    return r;
}
__device__ __forceinline__ unsigned bf2_pack(f32x2 v) { return f2bf_pk(v[0], v[1]); }
// max of the two signed 16-bit halves with `lo` in both: lo = 0 is ReLU on a packed bf16 pair (a negative bf16 is a negative
// int16; rounding is monotonic and keeps the sign, so relu(round(t)) == round(relu(t))), lo = -32768 is the identity.
// Not the bits of the scalar fmaxf path in two corners: -0.0 becomes +0.0 (equal as an MFMA operand and in
// every sum), and a NaN survives with its sign bit clear / becomes 0 with it set, where fmaxf(NaN, 0) = 0 -- a NaN activation
// means the step has diverged either way; the cross-kernel bit tests use finite inputs.
__device__ __forceinline__ unsigned bf2_floor(unsigned w, short lo) {
    s16x2 a = *reinterpret_cast<const s16x2*>(&w);
    const s16x2 b = {lo, lo};
    a = __builtin_elementwise_max(a, b);
    return *reinterpret_cast<const unsigned*>(&a);
}
__device__ __forceinline__ void bf2_unpack4(const uint4& w, f32x2 (&f)[4]) {
    f[0] = bf2_unpack(w.x); f[1] = bf2_unpack(w.y); f[2] = bf2_unpack(w.z); f[3] = bf2_unpack(w.w);
}

// ---- FOLDED BN-BACKWARD APPLY (fpd_conv_t.fold_x): coefficients of channel c into s_fold [3][C] ---------------------------------
// dy = gamma*is*(g - m1 - xhat*m2), xhat = (u - mu)*is  ==  A g + B u + D, formed in fp64 from the forward statistics (braw: the
// requested fold_bn) and the two BN-backward sums (fs1, fs2: the requested fold_stats).  The affine parameters' gradients fall out
// of the two sums: one block of the launch (writes_affine) stores them.  The expressions are kept as they are: fp64 contraction
// decides the bits.  (conv_tile keeps a copy of this text: see there.)
__device__ __forceinline__ void fold_coef(const fpd_conv_t& a, const BnRaw& braw, const StatRaw& fs1, const StatRaw& fs2, const double count,
                                          float* s_fold, const int C, const int c, const bool writes_affine) {
    const double s1 = stat_resolve(braw.s1), s2 = stat_resolve(braw.s2), b1 = stat_resolve(fs1), b2 = stat_resolve(fs2);
    const double cnt = count, mu = s1 / cnt;
    double var = s2 / cnt - mu * mu;
    if (var < 0.0) var = 0.0;
    const double is = 1.0 / sqrt(var + (double)braw.eps), gi = (double)braw.g * is;
    const double m1 = b1 / cnt, m2 = b2 / cnt;
    s_fold[c] = (float)gi;
    s_fold[C + c] = (float)(-gi * is * m2);
    s_fold[2 * C + c] = (float)(gi * (mu * is * m2 - m1));
    if (writes_affine) {
        if (a.fold_dgamma != nullptr) a.fold_dgamma[c] = (float)b2;
        if (a.fold_dbeta != nullptr) a.fold_dbeta[c] = (float)b1;
    }
}

// ---- table prologue of a 512-thread block: the table chains (loads -> fp64 -> LDS) on different waves ---------------------------
// Threads [0, C) own the prologue BN or the fold coefficients, [128, 128 + K) the epilogue BN of a data gradient, [256, 256 + K)
// the bias(es).  request() only issues the loads -- the kernel calls it before its long loads (weights, first tile) --, resolve()
// does the arithmetic on what arrived and writes the LDS tables behind them; the kernel keeps a sched_barrier around both.
// Branch shape as in bn_request (common.h): every field a role needs is assigned exactly once in its branch and nothing is
// written first as a default -- a default written in front (the biases, say) is sunk by hipcc behind the other branches'
// loads, where it needs vmcnt(0).
template <int C, int K, bool BWD, bool SKIP>
struct StreamTables {
    BnRaw braw;
    StatRaw fs1, fs2;
    float bias_raw, bias2_raw;
    int te, tb;
    bool r_bn, r_fold, r_epi, r_bias;

    __device__ __forceinline__ void request(const fpd_conv_t& a, const int tid, const bool has_bn, const bool fold) {
        te = tid - 128; tb = tid - 256;
        r_bn = has_bn && tid < C;
        r_fold = fold && tid < C;
        r_epi = BWD && te >= 0 && te < K;
        r_bias = tb >= 0 && tb < K;
        if (r_bn) bn_request(a.bn, tid, C, braw);
        else if (r_fold) {
            bn_request(a.fold_bn, tid, C, braw);
            stat_request(a.fold_stats, C, 0, tid, fs1);
            stat_request(a.fold_stats, C, 1, tid, fs2);
        }
        else if (r_epi) bn_request(a.epi_bn, te, K, braw);
        else if (r_bias) {
            bias_raw = 0.f; if (a.bias != nullptr) bias_raw = a.bias[tb];
            if constexpr (SKIP) { bias2_raw = 0.f; if (a.bias2 != nullptr) bias2_raw = a.bias2[tb]; }
        }
    }
    // M: pixels of the convolution (the count of every statistic); s_bias2: SKIP only
    __device__ __forceinline__ void resolve(const fpd_conv_t& a, const int tid, const int M, const bool writes_affine, float* s_scale,
                                            float* s_shift, float* s_fold, float* s_epi, float* s_bias, float* s_bias2) {
        if (r_bn) {
            float sc, sh, mu, is;
            bn_resolve(braw, (double)M, sc, sh, mu, is);
            s_scale[tid] = sc;
            s_shift[tid] = sh;
        } else if (r_fold) {
            fold_coef(a, braw, fs1, fs2, (double)M, s_fold, C, tid, writes_affine);
        } else if (r_epi) {
            float sc, sh, mu, is;
            bn_resolve(braw, (double)M, sc, sh, mu, is);
            s_epi[te] = sc; s_epi[K + te] = sh; s_epi[2 * K + te] = mu; s_epi[3 * K + te] = is;
        } else if (r_bias) {
            s_bias[tb] = bias_raw;
            if constexpr (SKIP) s_bias2[tb] = bias2_raw;
        }
    }
};

// ---- per-channel epilogue on one 16-byte vector (8 channels of one pixel; a lane always holds chunk kch) --------------------------
// epilogue BN of the lane's 8 output channels, as pairs (re-read from the LDS in the phase that uses them: the registers are needed
// for the accumulators and the vectors in flight)
struct EpiTab { f32x2 sc[4], sh[4], mu[4], is[4]; };
template <int K>
__device__ __forceinline__ void epi_tab_read(const float* s_epi, const int kch, EpiTab& t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        t.sc[e] = *reinterpret_cast<const f32x2*>(s_epi + kch * 8 + 2 * e);
        t.sh[e] = *reinterpret_cast<const f32x2*>(s_epi + K + kch * 8 + 2 * e);
        t.mu[e] = *reinterpret_cast<const f32x2*>(s_epi + 2 * K + kch * 8 + 2 * e);
        t.is[e] = *reinterpret_cast<const f32x2*>(s_epi + 3 * K + kch * 8 + 2 * e);
    }
}
// BWD, one pair of channels (e = 0..3 of the vector): ReLU mask of the forward tensor xw (it commutes with the rounding) on the
// gradient ow, then the two BatchNorm-backward sums of the stored (rounded) gradient.  Returns z, the forward BatchNorm of xw:
// conv_c1's fused weight gradient re-forms the forward operand from it.  (Per pair, all by value: as ONE function on the whole
// vector, arrays by reference, hipcc scheduled conv_c1's plain data gradients with 7 more instructions per tile.)
__device__ __forceinline__ f32x2 epi_bwd_pair(unsigned& ow, const unsigned xw, const EpiTab& t, const int e, const float relu_gate, f32x2& F1, f32x2& F2) {
    const f32x2 xv = bf2_unpack(xw);
    const f32x2 z = __builtin_elementwise_fma(xv, t.sc[e], t.sh[e]);
    const unsigned keep = (z[0] > relu_gate ? 0x0000ffffu : 0u) | (z[1] > relu_gate ? 0xffff0000u : 0u);
    ow &= keep;
    const f32x2 g = bf2_unpack(ow);
    F1 += g;
    F2 = __builtin_elementwise_fma(g, (xv - t.mu[e]) * t.is[e], F2);
    return z;
}
// forward: sums of the result shifted by the wave's common shift CS (the value of its first pixel)
__device__ __forceinline__ void epi_fwd_step(const unsigned (&ow)[4], const f32x2 (&CS)[4], f32x2 (&F1)[4], f32x2 (&F2)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const f32x2 d = bf2_unpack(ow[e]) - CS[e];
        F1[e] += d;
        F2[e] = __builtin_elementwise_fma(d, d, F2[e]);
    }
}
// one vector at a time, its sums formed HERE: hipcc otherwise sinks the statistics arithmetic of all vectors behind the loop and
// keeps every unpacked operand alive until then (more registers than the kernel has)
__device__ __forceinline__ void epi_sums_fence(f32x2 (&F1)[4], f32x2 (&F2)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(F1[e]), "+v"(F2[e]));
    __builtin_amdgcn_sched_barrier(0);
}

// ---- statistics: one flush per block of NW waves x 64 lanes (512 threads) --------------------------------------------------------
// A lane holds fp32 partial sums of 8 channels over its pixels (forward: shifted by the wave's common shift CS; backward {sum dz,
// sum dz * xhat}); fixed-order fp64 sums per channel, exact limbs out.  rec: LDS the waves' tiles occupied, [NW][64][16] records +
// [NW][K] shifts + [NPART][2 K] doubles.  tiles_of_wave(wv): 32-pixel tiles wave wv of this block has processed (forward only).
// Stage A (all threads): thread (part, which, ch) sums the records of NPW waves in a fixed order in fp64 and un-shifts them;
// stage B: the parts in order, one exact pair of limbs per (sum, channel) out.  (One thread per sum over all eight waves took
// 6.4 k cycles at the end of every block: stamps, round 6.)
template <int NW, int K, bool BWD, typename TilesOfWave>
__device__ __forceinline__ void stream_stats_flush(float* rec, fpd_stat_t* st, const f32x2 (&F1)[4], const f32x2 (&F2)[4], const f32x2 (&CS)[4],
                                                   const int wave, const int lane, const int tid, TilesOfWave tiles_of_wave) {
    constexpr int KV = K / 8;
    __syncthreads();                                      // every wave is done with its tiles
    float* shf = rec + NW * 64 * 16;                      // [NW][K]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        *reinterpret_cast<f32x2*>(rec + (wave * 64 + lane) * 16 + 2 * e) = F1[e];
        *reinterpret_cast<f32x2*>(rec + (wave * 64 + lane) * 16 + 8 + 2 * e) = F2[e];
    }
    if (!BWD && lane < KV) {
#pragma unroll
        for (int e = 0; e < 4; ++e) *reinterpret_cast<f32x2*>(shf + wave * K + lane * 8 + 2 * e) = CS[e];
    }
    __syncthreads();
    constexpr int NPART = 512 / (2 * K) > NW ? NW : 512 / (2 * K);      // 2 (K = 128), 4 (K = 64), 8 (K = 32)
    constexpr int NPW = NW / NPART;
    double* s_part = reinterpret_cast<double*>(shf + NW * K);           // [NPART][2 K]
    {
        const int part = tid / (2 * K), rem = tid % (2 * K);
        const int ch = rem % K, which = rem / K;          // which: 0 = first sum, 1 = second
        const int chunk = ch >> 3, e = ch & 7;
        if (part < NPART) {
            double tot = 0.0;
#pragma unroll
            for (int q = 0; q < NPW; ++q) {
                const int wv = part * NPW + q;
                double t1 = 0.0, t2 = 0.0;
#pragma unroll
                for (int jj = 0; jj < 64 / KV; ++jj) {
                    const float* rp = rec + (wv * 64 + chunk + KV * jj) * 16;
                    t1 += (double)rp[e];
                    t2 += (double)rp[8 + e];
                }
                if (BWD) tot += which ? t2 : t1;
                else {
                    const double c = (double)shf[wv * K + ch], nn = 32.0 * tiles_of_wave(wv);
                    tot += which ? (t2 + 2.0 * c * t1 + nn * c * c) : (t1 + nn * c);
                }
            }
            s_part[part * 2 * K + rem] = tot;
        }
    }
    __syncthreads();
    if (tid < 2 * K) {
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < NPART; ++q) tot += s_part[q * 2 * K + tid];
        stat_atomic_add(st, K, tid / K, tid % K, tot);
    }
}
