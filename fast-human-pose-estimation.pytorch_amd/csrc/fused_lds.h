// Dynamic-LDS layouts of the two fused teacher kernels (bneck_fused.hip, head_fused.hip), each stated ONCE: the device body carves
// its regions from these constants and the launcher sizes the launch with bytes(), so a change to a layout cannot leave a host
// formula behind and overrun the LDS without any error.  Plain constexpr C++ (no HIP header): tests/native/fused_lds_host.cpp
// includes it and walks every shape of the kernels' domains on the host.  Strides are bf16 elements unless they say otherwise.
#pragma once
#include <algorithm>
#include <cstddef>

// bneck_eval_body<P>: folded tables | a2 image (a3 aliases its dead rows) | R2, which the phases use in turn
template <int P>
struct BneckLds {
    static constexpr int C = 2 * P;
    static constexpr int TAB = 3 * C + 4 * P;            // floats: sc1[C] sh1[C] | sc2[P] sh2'[P] | sc3[P] sh3'[P] | b3[C]
    static constexpr int LDX = 64 + 8;                   // phase-A staging rows
    static constexpr int LD2 = P + 8;                    // a2 / a3 rows
    static constexpr int CW = 32 * (P / 64);             // channels per wave per step
    static constexpr int LST = CW + 4;                   // epilogue staging rows (fp32 elements)
    static constexpr int ASTG = (128 + P) * LDX;         // one phase-A staging buffer: x chunk [128][LDX] + w1 chunk [P][LDX]
    static constexpr int RING = P * P;                   // one [P][P] weight tile of phases B/C (LDS-DMA: rows are unpadded)
    // R2: two staging buffers (phase A) / two weight tiles (phases B, C) / eight wave-private [32][LST] fp32 tiles (epilogue)
    static constexpr size_t R2 = std::max({(size_t)2 * ASTG * 2, (size_t)2 * RING * 2, (size_t)8 * 32 * LST * 4});
    // a2 image: rows of W + 2 pixels.  Tiles made of whole images keep the plain halo tile, otherwise a ring of two half-slots of
    // nrows = 128 / W rows; behind the rows 3 zero pixels (the column tap offset is added to a redirected address too).
    static constexpr bool whole(int H, int W) { return 128 % (H * W) == 0; }
    static constexpr int irows(bool whole, int nrows) { return whole ? nrows + 2 : 2 * nrows; }
    static constexpr int image_px(int irows, int W) { return irows * (W + 2) + 3; }
    static constexpr size_t bytes(int H, int W) {
        return (size_t)TAB * sizeof(float) + (size_t)image_px(irows(whole(H, W), 128 / W), W) * LD2 * 2 + R2;
    }
};

// head_eval_kernel<C>: folded tables | activation image sA | score image sS | two weight buffers sW
template <int C>
struct HeadLds {
    static constexpr int TAB = 3 * C + 32;               // floats: sc[C] sh'[C] | b_score[32] | b_out[C]
    static constexpr int LDX = 64 + 8;                   // [.][64]-chunk rows
    static constexpr int LDA = C + 8;                    // activation image rows
    static constexpr int LDSC = 24;                      // score image rows (16 channels + pad)
    static constexpr int CW = 64;                        // channels per wave per epilogue round
    static constexpr int LST = CW + 4;                   // epilogue staging rows (fp32 elements)
    static constexpr int IMG = 128 * LDA;                // sA
    static constexpr int SCORE = 128 * LDSC;             // sS
    static constexpr int WTILE = C * LDX;                // one weight buffer
    static_assert(2 * 128 * LDX <= IMG, "GEMM1's two [128][LDX] staging buffers alias the activation image");
    static_assert(32 * LDA <= WTILE, "the [32][LDA] score-weight tile aliases one weight buffer");
    static_assert(8 * 32 * LST * 4 <= 2 * WTILE * 2, "the epilogue's wave-private fp32 tiles alias the weight buffers");
    static constexpr size_t bytes() { return (size_t)TAB * sizeof(float) + (size_t)(IMG + SCORE + 2 * WTILE) * 2; }
};
