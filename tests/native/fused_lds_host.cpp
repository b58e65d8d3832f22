// Host program: the dynamic-LDS sizes that csrc/fused_lds.h describes, against the formulas the launchers of bneck_fused.hip and
// head_fused.hip carried before the layouts were stated once (kept here word for word), over every shape of the kernels' domains:
// P in {64, 128}, W a power of two in 4..64, every H up to 512 with H * W a multiple or a divisor of 128.  Also that each region
// R2 is used for fits inside it.  Prints "<n> shapes ok" and returns 0, or the first difference and 1.
#include <algorithm>
#include <cstdio>

#include "fused_lds.h"

template <int P>
static size_t old_bneck_lds_bytes(int H, int W) {
    constexpr int C = 2 * P, LD2 = P + 8, LDX = 72, CW = 32 * (P / 64);
    int logW = 0;
    while ((1 << logW) < W) ++logW;
    const int nrows = 128 >> logW, WP = W + 2;
    const bool whole = (128 % (H * W)) == 0;
    const int irows = whole ? nrows + 2 : 2 * nrows;          // a2 image: plain halo tile / ring of two half-slots
    const size_t r2 = std::max({(size_t)2 * P * LD2 * 2, (size_t)2 * (128 + P) * LDX * 2, (size_t)8 * 32 * (CW + 4) * 4});
    return (size_t)(3 * C + 4 * P) * sizeof(float) + (size_t)(irows * WP + 3) * LD2 * 2 + r2;
}

static size_t old_head_lds_bytes() {
    constexpr int C = 256, LDX = 72, LDA = C + 8;
    return (size_t)(3 * C + 32) * sizeof(float) + (size_t)128 * LDA * 2 + (size_t)128 * 24 * 2 + (size_t)2 * C * LDX * 2;
}

template <int P>
static int walk(int& n) {
    using L = BneckLds<P>;
    static_assert(L::R2 >= (size_t)2 * L::ASTG * 2 && L::R2 >= (size_t)2 * L::RING * 2 && L::R2 >= (size_t)8 * 32 * L::LST * 4, "R2 holds each of its uses");
    static_assert(L::TAB % 4 == 0 && (L::LD2 * 2) % 16 == 0 && L::R2 % 16 == 0, "regions start on 16-byte boundaries");
    for (int W = 4; W <= 64; W *= 2)
        for (int H = 1; H <= 512; ++H) {
            const int hw = H * W;
            if (hw % 128 != 0 && 128 % hw != 0) continue;
            const size_t now = L::bytes(H, W), old = old_bneck_lds_bytes<P>(H, W);
            if (now != old) {
                std::printf("bneck P=%d H=%d W=%d: %zu bytes, the launcher had %zu\n", P, H, W, now, old);
                return 1;
            }
            ++n;
        }
    return 0;
}

int main() {
    int n = 0;
    if (walk<64>(n) || walk<128>(n)) return 1;
    if (HeadLds<256>::bytes() != old_head_lds_bytes()) {
        std::printf("head: %zu bytes, the launcher had %zu\n", HeadLds<256>::bytes(), old_head_lds_bytes());
        return 1;
    }
    std::printf("%d shapes ok\n", n + 1);
    return 0;
}
