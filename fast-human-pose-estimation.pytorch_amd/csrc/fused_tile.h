// Device pieces shared by the two fused teacher kernels (bneck_fused.hip, head_fused.hip).  Both work on 128-pixel tiles with
// 8 wave64 (4 pixel groups of 32 x 2 channel halves) and "transposed" MFMAs, so a lane holds 4 CONSECUTIVE channels of one pixel
// per register quad: the sum of two bf16 vectors rounded once, the activation store relu(bn(acc)) -> bf16 -> LDS row, and the two
// halves of the wave-private staged epilogue.  Everything here is __forceinline__ and compiles to what the kernels held as their
// own text (profiles/fused_tile_isa.txt); the loops over steps, tiles and output vectors, the tile addressing,
// the barriers and the pipeline order stay in the kernels.  So does the request of the residual rows, and the epilogue's second
// half is shared per VECTOR: with the pixel index m0 + 32 q + px formed inside a shared function, hipcc no longer hoists its
// tile-invariant part: an MFMA block of every kernel gets one more v_or_b32 and the UPADD kernels take more registers.
#pragma once
#include "common.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // native vector: typed loads/stores (a uint4 struct
                                                                  // copy is a memcpy, which keeps its array in scratch)

// round_bf16(a + b) of 8 bf16: the up-add the hourglass forms in front of a Bottleneck, bit for bit what FPD_EW_UPADD_FWD stores
__device__ __forceinline__ u32x4 bf16x8_sum(const u32x4 a, const u32x4 b) {
    float v[8], u[8];
    DT<bf16_t>::unpack(make_uint4(a[0], a[1], a[2], a[3]), v);
    DT<bf16_t>::unpack(make_uint4(b[0], b[1], b[2], b[3]), u);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] + u[e];
    const uint4 o = DT<bf16_t>::pack(v);
    const u32x4 ov = {o.x, o.y, o.z, o.w};
    return ov;
}

// relu(sc * acc + sh) -> bf16 -> the lane's pixel row `dst` of an LDS image, as packed 8-byte writes: TN 32-channel MFMA tiles
// from channel c0 (s_sc / s_sh: the folded BN tables, the conv bias inside sh)
template <int TN>
__device__ __forceinline__ void act_store(const f32x16 (&acc)[TN], const float* s_sc, const float* s_sh, const int c0, const int lane, bf16_t* dst) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) {
            const int c = c0 + tn * 32 + 8 * gi + 4 * (lane >> 5);
            const f32x4 sc = *reinterpret_cast<const f32x4*>(s_sc + c);
            const f32x4 sh = *reinterpret_cast<const f32x4*>(s_sh + c);
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(acc[tn][4 * gi + e], sc[e], sh[e]), 0.f);
            *reinterpret_cast<uint2*>(dst + c) = make_uint2(f2bf_pk(v[0], v[1]), f2bf_pk(v[2], v[3]));
        }
}

// ---- epilogue of a wave: its [32 px][CW] output slice goes through a wave-private [32 px][CW + 4] fp32 tile `stage` and comes
//      back as 32 * CW / 8 / 64 whole 16-byte vectors per lane ----
// first half: the accumulators of TN = CW / 32 MFMA tiles -> stage
template <int TN>
__device__ __forceinline__ void epi_stage(const f32x16* acc, float* stage, const int lane) {
    constexpr int LST = 32 * TN + 4;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[tn][4 * gi + e];
            *reinterpret_cast<f32x4*>(stage + (lane & 31) * LST + tn * 32 + 8 * gi + 4 * (lane >> 5)) = v;
        }
}
// second half, one 16-byte vector: 8 channels of a pixel read back from its row of the tile (srow), + bias + residual in fp32, ONE rounding
__device__ __forceinline__ uint4 epi_vec(const float* srow, const float* bias, const u32x4 r) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(srow);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(srow + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bias);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(bias + 4);
    float res[8], o[8];
    DT<bf16_t>::unpack(make_uint4(r[0], r[1], r[2], r[3]), res);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o[e] = v0[e] + b0[e] + res[e];
        o[4 + e] = v1[e] + b1[e] + res[4 + e];
    }
    return DT<bf16_t>::pack(o);
}
