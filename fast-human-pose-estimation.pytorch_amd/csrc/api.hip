// C-ABI entry points (include/fpd_amd.h): argument validation, backend dispatch, execution plan,
// hipGraph capture/replay, HIP-event timing helpers.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "conv_dispatch.h"

int g_fpd_backend = FPD_BACKEND_MFMA;
static thread_local char g_err[512] = "";

// ---- launch log (common.h FPD_LAUNCH) ----
static FILE* g_launch_log_file = nullptr;
static bool launch_log_open() {
    const char* path = getenv("FPD_LAUNCH_LOG");
    if (path == nullptr || path[0] == 0) return false;
    g_launch_log_file = fopen(path, "w");
    if (g_launch_log_file == nullptr) fprintf(stderr, "[fpd_amd] FPD_LAUNCH_LOG: cannot open %s\n", path);
    return g_launch_log_file != nullptr;
}
bool g_fpd_launch_log = launch_log_open();
static thread_local char g_op_tag[256] = "-";          // the plan op being issued (set by fpd_plan_run / fpd_plan_run_op)
void fpd_log_launch(const char* kernel, const dim3& grid, const dim3& block) {
    if (g_launch_log_file == nullptr) return;
    fprintf(g_launch_log_file, "%s\t%u\t%u\t%s\n", kernel, grid.x * grid.y * grid.z, block.x * block.y * block.z, g_op_tag);
    fflush(g_launch_log_file);
}

int fpd_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fpd_fail(-100 - (int)e, "kernel launch failed: %s", hipGetErrorString(e));
    return 0;
}

static int validate_conv_dims(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int P, int Q) {
    FPD_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && R > 0 && S > 0 && stride > 0 && pad >= 0,
                "conv: non-positive dimension");
    FPD_REQUIRE(P == (H + 2 * pad - R) / stride + 1 && Q == (W + 2 * pad - S) / stride + 1,
                "conv: output %dx%d inconsistent with input %dx%d k=%dx%d stride=%d pad=%d", P, Q, H, W, R, S, stride, pad);
    FPD_REQUIRE((int64_t)N * H * W * C < (1ll << 31) && (int64_t)N * P * Q * K < (1ll << 31), "conv: tensor too large for 32-bit indexing");
    return 0;
}

extern "C" {

const char* fpd_last_error(void) { return g_err; }
int fpd_abi_version(void) { return FPD_ABI_VERSION; }
int64_t fpd_stats_words(int32_t channels) { return FPD_STATS_WORDS(channels); }
int fpd_set_backend(int32_t backend) {
    const int prev = g_fpd_backend;
    if (backend == FPD_BACKEND_MFMA || backend == FPD_BACKEND_NAIVE || backend == FPD_BACKEND_MFMA_GENERIC) g_fpd_backend = backend;
    return prev;
}

static int g_wgrad_tile_only = 0;      // tests: fail instead of falling through to the generic weight-gradient kernels

int fpd_set_option(const char* name, int32_t value) {
    FPD_REQUIRE(name, "set_option: null name");
    if (!strcmp(name, "conv_pp")) return fpd_conv_pp_option(0, value);
    if (!strcmp(name, "conv_pp_blocks")) return fpd_conv_pp_option(1, value);
    if (!strcmp(name, "conv_c1")) return fpd_conv_c1_option(0, value);
    if (!strcmp(name, "conv_c1_blocks")) return fpd_conv_c1_option(1, value);
    if (!strcmp(name, "conv_c1_launches")) return fpd_conv_c1_option(2, value);      // (read-only: launches served so far)
    if (!strcmp(name, "conv_skip")) return fpd_conv_c1_option(3, value);             // second 1x1 source (fpd_conv_t.x2) offered at all
    if (!strcmp(name, "stem_act")) return fpd_stem_s2d_option(0, value);             // eval-mode BN + ReLU in the stem's epilogue (fpd_stem_t.act)
    if (!strcmp(name, "stem_blocks")) return fpd_stem_s2d_option(1, value);          // grid / slab cap of the persistent stem kernels (tests: several tiles per block), 0 = none
    if (!strcmp(name, "stem_s2d_launches")) return fpd_stem_s2d_option(2, value);    // (read-only: forward + weight-gradient launches stem_s2d.hip has served)
    if (!strcmp(name, "stem_mfma_launches")) return fpd_stem_mfma_launches();        // (read-only: ... stem_mfma.hip has served; neither moved: the direct kernels)
    if (!strcmp(name, "ew_merge")) return fpd_ew_merge_option(value < 0 ? 0 : value);      // BN-backward applies inside the pool backward (fpd_ew_merge_t) offered at all
    if (!strcmp(name, "ew_merge_blocks")) return fpd_ew_merge_blocks_option(value);      // their grid cap (tests: several windows per thread on small tensors)
    if (!strcmp(name, "ew_blocks")) return fpd_ew_blocks_option(value);      // grid cap of the plain elementwise, pair and affsum launches (tests: several trips per thread), 0 = none
    if (!strcmp(name, "conv_c3")) return fpd_conv_c3_option(0, value);
    if (!strcmp(name, "conv_c3_blocks")) return fpd_conv_c3_option(1, value);
    if (!strcmp(name, "conv_c3_launches")) return fpd_conv_c3_option(2, value);
    if (!strcmp(name, "conv_tile_launches")) return fpd_conv_tile_launches();        // (read-only: launches conv_tile.hip has served)
    if (!strcmp(name, "wgrad_tile_launches")) return fpd_wgrad_tile_launches();      // (read-only: launches of wgrad_tile_kernel; those handed to wgrad3 are not counted)
    if (!strcmp(name, "wgrad3_launches")) return fpd_wgrad3_launches();              // (read-only: launches served by wgrad3.hip)
    if (!strcmp(name, "bneck_blocks")) return fpd_bneck_blocks_option(value);
    if (!strcmp(name, "bneck_upadd")) return fpd_bneck_upadd_option(value);          // up-add formed on load (fpd_bneck_t.x2) offered at all
    if (!strcmp(name, "head_blocks")) return fpd_head_blocks_option(value);
    if (!strcmp(name, "wgrad_tile_only")) { g_wgrad_tile_only = value; return 0; }
    return fpd_fail(-2, "set_option: unknown option '%s'", name);
}

int fpd_abi_sizeof(const char* n) {
#define SZ(T) if (!strcmp(n, #T)) return (int)sizeof(T)
    SZ(fpd_bn_t); SZ(fpd_conv_t); SZ(fpd_wgrad_t); SZ(fpd_stem_t); SZ(fpd_ew_t); SZ(fpd_loss_t); SZ(fpd_adam_t);
    SZ(fpd_wprep_entry_t); SZ(fpd_bnupd_entry_t); SZ(fpd_memset_t); SZ(fpd_table_t); SZ(fpd_wreduce_entry_t); SZ(fpd_bneck_t); SZ(fpd_conv_pair_t); SZ(fpd_bneck_pair_t); SZ(fpd_ew_pair_t); SZ(fpd_pck_t); SZ(fpd_head_t); SZ(fpd_affsum_t); SZ(fpd_layout_t);
    SZ(fpd_conv_f8_t); SZ(fpd_wquant_entry_t); SZ(fpd_flipmerge_t); SZ(fpd_finalpreds_t); SZ(fpd_targets_t); SZ(fpd_warp_src_t); SZ(fpd_warp_t);
    SZ(fpd_loss_ohkm_t); SZ(fpd_sgd_t); SZ(fpd_ew_merge_t); SZ(fpd_loss_kl_t); SZ(fpd_ema_t); SZ(fpd_grad_clip_t); SZ(fpd_grad_accum_t); SZ(fpd_adamw_t);
    SZ(fpd_aug_img_t); SZ(fpd_aug_db_t); SZ(fpd_aug_crop_t); SZ(fpd_augment_t); SZ(fpd_warp_aug_t); SZ(fpd_targets_w_t); SZ(fpd_targets_unbiased_t);
    SZ(fpd_oks_nms_t); SZ(fpd_coco_match_t); SZ(fpd_coco_accum_t); SZ(fpd_val_post_t); SZ(fpd_dark_t);
    SZ(fpd_vis_minmax_t); SZ(fpd_vis_max_preds_t); SZ(fpd_vis_joints_grid_t); SZ(fpd_vis_heatmap_grid_t);
#undef SZ
    return -1;
}

static int validate_conv(const fpd_conv_t* a) {
    FPD_REQUIRE(a && a->x && a->w && a->y, "conv: null pointer");
    int rc = validate_conv_dims(a->N, a->H, a->W, a->C, a->K, a->R, a->S, a->stride, a->pad, a->P, a->Q);
    if (rc) return rc;
    FPD_REQUIRE(a->dtype == FPD_F32 || a->dtype == FPD_BF16, "conv: bad dtype %d", a->dtype);
    FPD_REQUIRE(a->bn.mode == FPD_BN_NONE || (a->bn.gamma && a->bn.beta), "conv: BN prologue without gamma/beta");
    FPD_REQUIRE(a->bn.mode != FPD_BN_TRAIN || a->bn.stats, "conv: train-mode BN without statistics");
    FPD_REQUIRE(a->bn.mode != FPD_BN_EVAL || (a->bn.running_mean && a->bn.running_var), "conv: eval-mode BN without running stats");
    FPD_REQUIRE(a->epi == FPD_EPI_PLAIN || (a->epi_x && a->epi_stats && a->epi_bn.mode == FPD_BN_TRAIN && a->epi_bn.stats),
                "conv: BNRELU_BWD epilogue needs epi_x, epi_stats and a train-mode epi_bn");
    FPD_REQUIRE(a->x2 == nullptr || (a->w2 != nullptr && a->C2 > 0), "conv: a second source (x2) needs w2 and C2");
    FPD_REQUIRE(a->x2 == nullptr || a->residual == nullptr, "conv: a second source (x2) and a residual exclude each other");
    return 0;
}

// ---- convolution backends, in dispatch order: the ONE place that states it.  Launches and queries walk this table. ----
constexpr unsigned ON_MFMA = 1u << FPD_BACKEND_MFMA, ON_GENERIC = ON_MFMA | 1u << FPD_BACKEND_MFMA_GENERIC, ON_ANY = ON_GENERIC | 1u << FPD_BACKEND_NAIVE;
struct ConvBackend {
    const char* name;
    unsigned backends;          // the g_fpd_backend values it is eligible under (bit set)
    int (*route)(const fpd_conv_t& a, const fpd_conv_t* b, ConvAsk ask, ConvRoute& r);      // nullptr: decides inside its launch; no fold, no slabs, no pairs
    int (*launch)(const fpd_conv_t& a, const fpd_conv_t* b, hipStream_t st);
};
static const ConvBackend g_conv_backends[] = {
    {"conv_c1", ON_MFMA, fpd_conv_c1_route, fpd_conv_c1_launch},            // big maps, 1x1: streaming kernel
    {"conv_c3", ON_MFMA, fpd_conv_c3_route, fpd_conv_c3_launch},            // big maps, 3x3 64 -> 64: strip kernel
    {"conv_pp", ON_MFMA, fpd_conv_pp_route, fpd_conv_pp_launch},            // big maps: persistent kernel
    {"conv_tile", ON_MFMA, fpd_conv_tile_route, fpd_conv_tile_launch},      // halo-tile kernel
    {"conv_mfma", ON_GENERIC, nullptr, [](const fpd_conv_t& a, const fpd_conv_t*, hipStream_t st) { return fpd_conv_mfma_launch(a, st); }},
    {"conv_smallc", ON_GENERIC, nullptr, [](const fpd_conv_t& a, const fpd_conv_t*, hipStream_t st) { return fpd_conv_smallc_launch(a, st); }},   // tiny input-channel counts (3, 17)
    {"conv_naive", ON_ANY, nullptr, [](const fpd_conv_t& a, const fpd_conv_t*, hipStream_t st) { return fpd_conv_naive_launch(a, st); }},
};
static bool eligible(unsigned backends) { return (backends >> g_fpd_backend & 1u) != 0; }

// The backend that serves the launch (b != nullptr: the pair launch) carrying `ask`, and what it offers there.  The walk ends at
// the first generic backend: whichever of them launches, it offers nothing.  nullptr: a pair that no kernel pairs.
static const ConvBackend* route_conv(const fpd_conv_t& a, const fpd_conv_t* b, ConvAsk ask, ConvRoute& r) {
    r = ConvRoute{false, 0, 0, false};
    for (const ConvBackend& e : g_conv_backends) {
        if (!eligible(e.backends)) continue;
        if (e.route == nullptr ? b == nullptr : e.route(a, b, ask, r) == 0) return &e;
    }
    return nullptr;
}

static int launch_conv(const fpd_conv_t& a, const fpd_conv_t* b, hipStream_t st) {
    ConvRoute r;
    const ConvBackend* e = route_conv(a, b, fpd_conv_ask(a, b), r);
    if (e == nullptr) {                  // not pairable: same result from two launches
        const int rc = launch_conv(a, nullptr, st);
        return rc ? rc : launch_conv(*b, nullptr, st);
    }
    // a fusion the fields ask for and the route does not offer: refused here, before any HIP call
    FPD_REQUIRE(!(a.wg_partial != nullptr && r.slabs_a == 0) && !(b != nullptr && b->wg_partial != nullptr && r.slabs_b == 0),
                "conv: the launch asks for a fused weight gradient (wg_partial), which its route (%s) does not offer; %s() reports 0 for it",
                e->name, b ? "fpd_conv_pair_fused_wgrad_partials" : "fpd_conv_fused_wgrad_partials");
    FPD_REQUIRE(r.folds || (a.fold_x == nullptr && (b == nullptr || b->fold_x == nullptr)),
                "conv: the launch asks for a folded BN-backward apply (fold_x), which its route (%s) does not offer; %s() reports 0 for it",
                e->name, b ? "fpd_conv_pair_fold_supported" : "fpd_conv_fold_supported");
    FPD_REQUIRE(r.skips || (a.x2 == nullptr && (b == nullptr || b->x2 == nullptr)),
                "conv: the launch carries a second 1x1 source (x2), which its route (%s) does not offer; fpd_conv_skip_supported() reports 0 for it", e->name);
    int rc = e->launch(a, b, st);
    for (++e; rc == 1 && e != std::end(g_conv_backends); ++e)      // a generic kernel declines inside its launch: on to the next one
        if (e->route == nullptr && eligible(e->backends)) rc = e->launch(a, b, st);
    return rc;
}

int fpd_conv_forward(const fpd_conv_t* a, fpd_stream_t stream) {
    int rc = validate_conv(a);
    if (rc) return rc;
    rc = launch_conv(*a, nullptr, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

// The queries answer for the launch as it will be made: `fold` / `wg` asked for, the other taken from the fields.
int fpd_conv_fold_supported(const fpd_conv_t* a) {
    ConvRoute r;
    if (!a || validate_conv(a) != 0) return 0;
    route_conv(*a, nullptr, ConvAsk{true, a->wg_partial != nullptr, a->x2 != nullptr}, r);
    return r.folds ? 1 : 0;
}
int fpd_conv_pair_fold_supported(const fpd_conv_pair_t* p) {
    ConvRoute r;
    if (!p || validate_conv(&p->a) != 0 || validate_conv(&p->b) != 0) return 0;
    if (route_conv(p->a, &p->b, ConvAsk{true, fpd_conv_ask(p->a, &p->b).wg, fpd_conv_ask(p->a, &p->b).skip}, r) != nullptr) return r.folds ? 1 : 0;
    return (fpd_conv_fold_supported(&p->a) && fpd_conv_fold_supported(&p->b)) ? 1 : 0;      // two single launches
}

// Which instantiation of the halo-tile kernel would run this launch (pair), asked of the kernel unit alone -- whether the dispatch
// gets as far as conv_tile is the business of the options and of the units in front of it.  The fold is asked for where fold_x is set.
int fpd_conv_tile_variant(const fpd_conv_t* a) {
    if (!a || validate_conv(a) != 0) return -1;
    return fpd_conv_tile_variant_of(*a, nullptr, fpd_conv_ask(*a, nullptr));
}
int fpd_conv_tile_pair_variant(const fpd_conv_pair_t* p) {
    if (!p || validate_conv(&p->a) != 0 || validate_conv(&p->b) != 0) return -1;
    return fpd_conv_tile_variant_of(p->a, &p->b, fpd_conv_ask(p->a, &p->b));
}

// (the second source is read from the fields: x2, w2, bias2, C2 as they will be launched)
int fpd_conv_skip_supported(const fpd_conv_t* a) {
    ConvRoute r;
    if (!a || validate_conv(a) != 0) return 0;
    route_conv(*a, nullptr, ConvAsk{a->fold_x != nullptr, a->wg_partial != nullptr, true}, r);
    return r.skips ? 1 : 0;
}

int fpd_conv_fused_wgrad_partials(const fpd_conv_t* a) {
    ConvRoute r;
    if (!a || validate_conv(a) != 0) return 0;
    route_conv(*a, nullptr, ConvAsk{a->fold_x != nullptr, true, a->x2 != nullptr}, r);
    return r.slabs_a;
}
int fpd_conv_pair_fused_wgrad_partials(const fpd_conv_pair_t* p, int32_t* n_a, int32_t* n_b) {
    FPD_REQUIRE(p && n_a && n_b, "conv_pair_fused_wgrad_partials: null pointer");
    *n_a = *n_b = 0;
    if (validate_conv(&p->a) != 0 || validate_conv(&p->b) != 0) return 0;
    ConvRoute r;
    route_conv(p->a, &p->b, ConvAsk{fpd_conv_ask(p->a, &p->b).fold, true, fpd_conv_ask(p->a, &p->b).skip}, r);      // (a pair that nothing pairs: two launches without the fusion)
    *n_a = r.slabs_a; *n_b = r.slabs_b;
    return 0;
}

int fpd_conv_f8_in_domain(const fpd_conv_t* c) { return (c && fpd_conv_f8_domain(*c)) ? 1 : 0; }
int fpd_conv_f8_variant(const fpd_conv_t* a) { return a ? fpd_conv_f8_variant_of(*a) : -1; }

int fpd_conv_forward_f8(const fpd_conv_f8_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a, "conv_f8: null pointer");
    int rc = validate_conv(&a->c);
    if (rc) return rc;
    FPD_REQUIRE(a->w8 && a->w8_scale, "conv_f8: null fp8 weights / scales");
    FPD_REQUIRE(((uintptr_t)a->w8 & 15) == 0, "conv_f8: w8 must be 16-byte aligned");
    rc = 1;
    if (g_fpd_backend == FPD_BACKEND_MFMA) rc = fpd_conv_tile_f8_launch(a->c, a->w8, a->w8_scale, (hipStream_t)stream);
    if (rc == 1) rc = launch_conv(a->c, nullptr, (hipStream_t)stream);      // outside the fp8 domain: the bf16 weights
    return rc ? rc : check_launch();
}

int fpd_weight_quant_f8(const fpd_wquant_entry_t* t, int32_t n, fpd_stream_t stream) {
    FPD_REQUIRE(n == 0 || t != nullptr, "weight_quant_f8: null table");
    int rc = fpd_weight_quant_f8_launch(t, n, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_conv_forward_pair(const fpd_conv_pair_t* p, fpd_stream_t stream) {
    FPD_REQUIRE(p, "conv_pair: null pointer");
    int rc = validate_conv(&p->a);
    if (rc) return rc;
    rc = validate_conv(&p->b);
    if (rc) return rc;
    FPD_REQUIRE(p->a.x2 == nullptr && p->b.x2 == nullptr, "conv_pair: a pair launch takes no second source (x2)");
    rc = launch_conv(p->a, &p->b, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

static int validate_bneck_bns(const fpd_bneck_t* a) {
    const fpd_bn_t* bns[3] = {&a->bn1, &a->bn2, &a->bn3};
    for (int i = 0; i < 3; ++i)
        FPD_REQUIRE(bns[i]->mode == FPD_BN_EVAL && bns[i]->relu && bns[i]->gamma && bns[i]->beta && bns[i]->running_mean &&
                    bns[i]->running_var, "bottleneck: bn%d must be an eval-mode BN+ReLU with running statistics", i + 1);
    return 0;
}

int fpd_bottleneck_fold(const fpd_bneck_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->folded, "bottleneck_fold: null pointer");
    int rc = validate_bneck_bns(a);
    if (rc) return rc;
    rc = fpd_bneck_fold_launch(*a, const_cast<float*>(a->folded), (hipStream_t)stream);
    if (rc == 1) return fpd_fail(-3, "bottleneck_fold: C=%d P=%d is outside the fused kernel's domain", a->C, a->P);
    return rc ? rc : check_launch();
}

int fpd_bottleneck_forward_pair(const fpd_bneck_pair_t* p, fpd_stream_t stream) {
    FPD_REQUIRE(p, "bottleneck_pair: null pointer");
    const fpd_bneck_t* ab[2] = {&p->a, &p->b};
    for (const fpd_bneck_t* a : ab) {
        FPD_REQUIRE(a->x && a->y && a->w1 && a->w2 && a->w3 && a->x != a->y, "bottleneck_pair: null pointer or y aliases x");
        FPD_REQUIRE(a->x2 == nullptr, "bottleneck_pair: a pair launch takes no low-branch source (x2)");
        FPD_REQUIRE((int64_t)a->N * a->H * a->W * a->C < ((int64_t)1 << 31), "bottleneck_pair: tensor too large for 32-bit indexing");
        int rc = validate_bneck_bns(a);
        if (rc) return rc;
    }
    int rc = fpd_bneck_fused_pair_launch(p->a, p->b, (hipStream_t)stream);
    if (rc == 1) {                       // not pairable: same result from two launches
        rc = fpd_bottleneck_forward(&p->a, stream);
        return rc ? rc : fpd_bottleneck_forward(&p->b, stream);
    }
    return rc ? rc : check_launch();
}

int fpd_bottleneck_forward(const fpd_bneck_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->x && a->y && a->w1 && a->w2 && a->w3, "bottleneck: null pointer");
    FPD_REQUIRE(a->x != a->y, "bottleneck: y must not alias x");
    FPD_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->C > 0 && a->P > 0, "bottleneck: bad dims");
    FPD_REQUIRE((int64_t)a->N * a->H * a->W * a->C < ((int64_t)1 << 31), "bottleneck: tensor too large for 32-bit indexing");
    int rc = validate_bneck_bns(a);
    if (rc) return rc;
    if (a->x2 != nullptr) {              // up-add on load: refused here, before any HIP call
        const char* why = fpd_bneck_upadd_why_not(*a);
        if (why) return fpd_fail(-3, "bottleneck: low-branch source (x2) with N=%d H=%d W=%d C=%d P=%d: %s; fpd_bneck_upadd_supported() reports 0 for it",
                                 a->N, a->H, a->W, a->C, a->P, why);
        FPD_REQUIRE(a->x2 != a->y, "bottleneck: y must not alias x2");
    }
    rc = fpd_bneck_fused_launch(*a, (hipStream_t)stream);
    if (rc == 1)
        return fpd_fail(-3, "bottleneck: shape N=%d H=%d W=%d C=%d P=%d dtype=%d is outside the fused kernel's domain",
                        a->N, a->H, a->W, a->C, a->P, a->dtype);
    return rc ? rc : check_launch();
}

int fpd_bneck_upadd_supported(const fpd_bneck_t* a) { return (a && fpd_bneck_upadd_why_not(*a) == nullptr) ? 1 : 0; }

// ---- weight-gradient backends, in dispatch order; partials: slabs the launch writes (0: it declines) ----
struct WgradBackend {
    unsigned backends;
    int (*partials)(const fpd_wgrad_t& a);
    int (*launch)(const fpd_wgrad_t& a, hipStream_t st);
};
static const WgradBackend g_wgrad_backends[] = {
    {ON_MFMA, fpd_wgrad_tile_partials, fpd_wgrad_tile_launch},      // halo-tile kernel (the only one under option wgrad_tile_only)
    {ON_GENERIC, fpd_wgrad_mfma_partials, fpd_wgrad_mfma_launch},
    {ON_GENERIC, fpd_wgrad_smallc_partials, fpd_wgrad_smallc_launch},
    {ON_ANY, fpd_wgrad_naive_partials, fpd_wgrad_naive_launch},
};

int fpd_conv_wgrad(const fpd_wgrad_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->x && a->dy && a->dw, "wgrad: null pointer");
    int rc = validate_conv_dims(a->N, a->H, a->W, a->C, a->K, a->R, a->S, a->stride, a->pad, a->P, a->Q);
    if (rc) return rc;
    FPD_REQUIRE(a->dtype == FPD_F32 || a->dtype == FPD_BF16, "wgrad: bad dtype %d", a->dtype);
    FPD_REQUIRE(a->partial == nullptr || a->partial_stride >= (int64_t)a->K * a->R * a->S * a->C + a->K,
                "wgrad: partial_stride %lld smaller than weight + bias", (long long)a->partial_stride);
    rc = 1;
    for (const WgradBackend& e : g_wgrad_backends) {
        FPD_REQUIRE(!(g_wgrad_tile_only && &e != g_wgrad_backends), "wgrad: option wgrad_tile_only is set and the halo-tile kernel declines N=%d H=%d W=%d C=%d K=%d R=%d", a->N, a->H, a->W, a->C, a->K, a->R);
        if (eligible(e.backends)) rc = e.launch(*a, (hipStream_t)stream);
        if (rc != 1) break;
    }
    return rc ? rc : check_launch();
}

int fpd_wgrad_tile_variant(const fpd_wgrad_t* a) {
    if (!a || validate_conv_dims(a->N, a->H, a->W, a->C, a->K, a->R, a->S, a->stride, a->pad, a->P, a->Q) != 0) return -1;
    return fpd_wgrad_tile_variant_of(*a);
}

/* slabs the kernel fpd_conv_wgrad() dispatches these dimensions to will write */
int fpd_wgrad_num_partials(const fpd_wgrad_t* a) {
    int n = 0;
    for (const WgradBackend& e : g_wgrad_backends)
        if (a && n == 0 && eligible(e.backends)) n = e.partials(*a);
    return n;
}

// ---- stem backends, in dispatch order (forward and weight gradient) ----
struct StemBackend {
    unsigned backends;
    bool (*takes_act)(const fpd_stem_t& a);      // the forward launch applies fpd_stem_t.act in its epilogue (nullptr: it never does)
    int (*forward)(const fpd_stem_t& a, hipStream_t st);
    int (*wgrad_partials)(const fpd_stem_t& a);
    int (*wgrad)(const fpd_stem_t& a, hipStream_t st);
};
static const StemBackend g_stem_backends[] = {
    {ON_MFMA, fpd_stem_forward_s2d_takes_act, fpd_stem_forward_s2d_launch, fpd_stem_wgrad_s2d_partials, fpd_stem_wgrad_s2d_launch},      // space-to-depth 4x4 form (round 5)
    {ON_MFMA, nullptr, fpd_stem_forward_mfma_launch, fpd_stem_wgrad_mfma_partials, fpd_stem_wgrad_mfma_launch},
    {ON_ANY, nullptr, fpd_stem_forward_launch, fpd_stem_wgrad_partials, fpd_stem_wgrad_launch},
};

int fpd_stem_wgrad_num_partials(const fpd_stem_t* a) {
    int n = 0;
    for (const StemBackend& e : g_stem_backends)
        if (a && n == 0 && eligible(e.backends)) n = e.wgrad_partials(*a);
    return n;
}

int fpd_wgrad_reduce(const fpd_wreduce_entry_t* t, int32_t n, int64_t max_elems, fpd_stream_t stream) {
    int rc = fpd_wreduce_launch(t, n, max_elems, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

// The first eligible backend decides: only the space-to-depth kernel applies `act`, and a launch it declines goes on to
// kernels that do not.
int fpd_stem_act_supported(const fpd_stem_t* a) {
    if (!a || a->act.mode != FPD_BN_EVAL || !a->act.gamma || !a->act.beta || !a->act.running_mean || !a->act.running_var || a->out_stats != nullptr) return 0;
    for (const StemBackend& e : g_stem_backends)
        if (eligible(e.backends)) return (e.takes_act != nullptr && e.takes_act(*a)) ? 1 : 0;
    return 0;
}

int fpd_stem_forward(const fpd_stem_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->x && a->w && a->bias && a->y, "stem: null pointer");
    FPD_REQUIRE(a->P == (a->H + 6 - 7) / 2 + 1 && a->Q == (a->W + 6 - 7) / 2 + 1, "stem: bad output size");
    FPD_REQUIRE(a->act.mode == FPD_BN_NONE || fpd_stem_act_supported(a) == 1,
                "stem: the launch asks for BN + ReLU in its epilogue (act), which is not offered for it; fpd_stem_act_supported() reports 0");
    int rc = 1;
    for (const StemBackend& e : g_stem_backends)
        if (rc == 1 && eligible(e.backends)) rc = e.forward(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_stem_wgrad(const fpd_stem_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->x && a->dy && a->dw, "stem wgrad: null pointer");
    FPD_REQUIRE(a->partial == nullptr || a->partial_stride >= (int64_t)a->K * 148, "stem wgrad: partial_stride %lld smaller than weight + bias",
                (long long)a->partial_stride);
    int rc = 1;
    for (const StemBackend& e : g_stem_backends)
        if (rc == 1 && eligible(e.backends)) rc = e.wgrad(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_affsum(const fpd_affsum_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->y, "affsum: null pointer");
    FPD_REQUIRE(a->nterms >= 1 && a->nterms <= FPD_AFFSUM_MAX, "affsum: %d terms (1..%d supported)", a->nterms, FPD_AFFSUM_MAX);
    FPD_REQUIRE(a->dtype == FPD_F32 || a->dtype == FPD_BF16, "affsum: bad dtype %d", a->dtype);
    for (int j = 0; j < a->nterms; ++j) {
        const int up = a->t[j].up;
        FPD_REQUIRE(a->t[j].x, "affsum: term %d has no input", j);
        FPD_REQUIRE((up == 1 || up == 2 || up == 4 || up == 8) && a->H % up == 0 && a->W % up == 0,
                    "affsum: term %d: up-sampling factor %d does not divide %dx%d", j, up, a->H, a->W);
        const fpd_bn_t& bn = a->t[j].bn;
        FPD_REQUIRE(bn.mode == FPD_BN_NONE || (bn.gamma && bn.beta), "affsum: term %d: BN without gamma/beta", j);
        FPD_REQUIRE(bn.mode != FPD_BN_TRAIN || bn.stats, "affsum: term %d: train-mode BN without statistics", j);
        FPD_REQUIRE(bn.mode != FPD_BN_EVAL || (bn.running_mean && bn.running_var), "affsum: term %d: eval-mode BN without running stats", j);
    }
    int rc = fpd_affsum_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_elementwise(const fpd_ew_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && (a->y || a->op == FPD_EW_BNRELU_BWD_R), "elementwise: null pointer");
    int rc = fpd_elementwise_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_ew_merge_supported(const fpd_ew_merge_t* a) { return (a && fpd_ew_merge_why_not(*a) == nullptr) ? 1 : 0; }
int fpd_ew_merge(const fpd_ew_merge_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a, "ew_merge: null pointer");
    int rc = fpd_ew_merge_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

static int validate_head(const fpd_head_t* a) {
    FPD_REQUIRE(a && a->y0 && a->score && a->w_fc && a->w_score, "head: null pointer");
    FPD_REQUIRE(a->next == nullptr || (a->x && a->w_fc2 && a->w_score2 && a->next != a->x && a->next != a->y0),
                "head: next needs x, w_fc2, w_score2 and must not alias an input");
    FPD_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && (int64_t)a->N * a->H * a->W * a->C < ((int64_t)1 << 31), "head: bad dims");
    FPD_REQUIRE(a->bn.mode == FPD_BN_EVAL && a->bn.relu && a->bn.gamma && a->bn.beta && a->bn.running_mean && a->bn.running_var,
                "head: bn must be an eval-mode BN+ReLU with running statistics");
    return 0;
}
int fpd_head_forward(const fpd_head_t* a, fpd_stream_t stream) {
    int rc = validate_head(a);
    if (rc) return rc;
    rc = fpd_head_fused_launch(*a, (hipStream_t)stream);
    if (rc == 1) return fpd_fail(-3, "head: C=%d J=%d dtype=%d is outside the fused kernel's domain", a->C, a->J, a->dtype);
    return rc ? rc : check_launch();
}
int fpd_head_fold(const fpd_head_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->folded, "head_fold: null pointer");
    FPD_REQUIRE(a->bn.mode == FPD_BN_EVAL && a->bn.gamma && a->bn.beta && a->bn.running_mean && a->bn.running_var, "head_fold: bn");
    int rc = fpd_head_fold_launch(*a, const_cast<float*>(a->folded), (hipStream_t)stream);
    if (rc == 1) return fpd_fail(-3, "head_fold: C=%d is outside the fused kernel's domain", a->C);
    return rc ? rc : check_launch();
}

int fpd_pck(const fpd_pck_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->out && a->target && a->counts && a->log && a->cursor, "pck: null pointer");
    FPD_REQUIRE(a->B > 0 && a->J > 0 && a->H > 0 && a->W > 0 && a->log_slots > 0, "pck: bad dims");
    FPD_REQUIRE(a->dtype == FPD_F32 || a->dtype == FPD_BF16, "pck: bad dtype %d", a->dtype);
    int rc = fpd_pck_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_flip_w(const float* x, float* y, int64_t rows, int32_t W, fpd_stream_t stream) {
    FPD_REQUIRE(x && y && x != y, "flip_w: null or aliased pointer");
    FPD_REQUIRE(rows > 0 && W > 0, "flip_w: bad dims");
    int rc = fpd_flip_w_launch(x, y, rows, W, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_flip_merge(const fpd_flipmerge_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->b && a->y && a->b != a->y, "flip_merge: null or aliased pointer");
    FPD_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->J > 0 && a->J <= FPD_MAX_JOINTS, "flip_merge: bad dims (J <= %d)", FPD_MAX_JOINTS);
    for (int j = 0; j < a->J; ++j) FPD_REQUIRE(a->src[j] >= 0 && a->src[j] < a->J, "flip_merge: src[%d] = %d out of range", j, a->src[j]);
    int rc = fpd_flip_merge_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_final_preds(const fpd_finalpreds_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->hm && a->coords && a->maxvals, "final_preds: null pointer");
    FPD_REQUIRE((a->trans == nullptr) == (a->preds == nullptr), "final_preds: trans and preds go together");
    FPD_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->J > 0, "final_preds: bad dims");
    int rc = fpd_final_preds_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_val_post(const fpd_val_post_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->a && a->center && a->scale && a->score && a->merged && a->all_preds && a->all_boxes, "val_post: null pointer");
    FPD_REQUIRE((const void*)a->merged != a->a && (const void*)a->merged != a->b, "val_post: merged aliases an input map");
    FPD_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->J > 0 && a->J <= FPD_MAX_JOINTS, "val_post: bad dims (J <= %d)", FPD_MAX_JOINTS);
    FPD_REQUIRE((int64_t)a->N * a->H * a->W * a->J < ((int64_t)1 << 31), "val_post: map too large");
    FPD_REQUIRE(a->row0 >= 0, "val_post: row0 = %lld is negative", (long long)a->row0);
    FPD_REQUIRE(a->row0 + a->N <= a->rows, "val_post: rows %lld..%lld outside the %lld result rows", (long long)a->row0,
                (long long)(a->row0 + a->N - 1), (long long)a->rows);
    FPD_REQUIRE(a->dtype == FPD_F32 || a->dtype == FPD_BF16, "val_post: bad dtype %d", a->dtype);
    if (a->b != nullptr)
        for (int j = 0; j < a->J; ++j) FPD_REQUIRE(a->src[j] >= 0 && a->src[j] < a->J, "val_post: src[%d] = %d out of range", j, a->src[j]);
    int rc = fpd_val_post_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_dark_refine(const fpd_dark_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->hm && a->taps, "dark_refine: null pointer (map or taps)");
    FPD_REQUIRE(a->ksize >= FPD_DARK_MIN_KSIZE && a->ksize <= FPD_DARK_MAX_KSIZE && (a->ksize & 1), "dark_refine: ksize = %d (odd, %d..%d)",
                a->ksize, FPD_DARK_MIN_KSIZE, FPD_DARK_MAX_KSIZE);
    FPD_REQUIRE(a->layout == FPD_DARK_NCHW || a->layout == FPD_DARK_NHWC, "dark_refine: bad layout %d", a->layout);
    FPD_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->J > 0 && a->J <= FPD_MAX_JOINTS, "dark_refine: bad dims (J <= %d)", FPD_MAX_JOINTS);
    FPD_REQUIRE((int64_t)a->H * a->W <= FPD_DARK_MAX_HW, "dark_refine: a %dx%d map does not fit LDS (H * W <= %d)", a->H, a->W, FPD_DARK_MAX_HW);
    FPD_REQUIRE((int64_t)a->N * a->H * a->W * a->J < ((int64_t)1 << 31), "dark_refine: map too large");
    FPD_REQUIRE((a->trans == nullptr) == (a->preds == nullptr), "dark_refine: trans and preds go together");
    const bool form_a = a->trans != nullptr;
    const bool form_b = a->center || a->scale || a->all_preds;
    FPD_REQUIRE(!(form_a && form_b), "dark_refine: both output forms given (trans/preds and center/scale/all_preds)");
    FPD_REQUIRE(form_a || form_b || a->coords, "dark_refine: no output (neither form, no coords)");
    if (form_b) {
        FPD_REQUIRE(a->center && a->scale && a->all_preds, "dark_refine: null pointer (center, scale and all_preds go together)");
        FPD_REQUIRE(a->row0 >= 0, "dark_refine: row0 = %lld is negative", (long long)a->row0);
        FPD_REQUIRE(a->row0 + a->N <= a->rows, "dark_refine: rows %lld..%lld outside the %lld result rows", (long long)a->row0,
                    (long long)(a->row0 + a->N - 1), (long long)a->rows);
    }
    int rc = fpd_dark_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

// ---- debug images (csrc/vis.hip) ----
static int validate_vis_map(const char* what, int dtype, int layout) {
    FPD_REQUIRE(layout == FPD_VIS_NCHW || layout == FPD_VIS_NHWC, "%s: bad layout %d", what, layout);
    FPD_REQUIRE(dtype == FPD_F32 || (dtype == FPD_BF16 && layout == FPD_VIS_NHWC), "%s: bad dtype %d for layout %d (NCHW maps are float32)",
                what, dtype, layout);
    return 0;
}
int fpd_vis_minmax(const fpd_vis_minmax_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->x && a->out, "vis_minmax: null pointer");
    FPD_REQUIRE(a->n > 0, "vis_minmax: n = %lld is not positive", (long long)a->n);
    FPD_REQUIRE((const void*)a->out != (const void*)a->x, "vis_minmax: out aliases the input");
    int rc = fpd_vis_minmax_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_vis_max_preds(const fpd_vis_max_preds_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->hm && a->preds && a->maxvals, "vis_max_preds: null pointer");
    FPD_REQUIRE(a->N > 0 && a->J > 0 && a->h > 0 && a->w > 0, "vis_max_preds: bad dims");
    FPD_REQUIRE((int64_t)a->N * a->J * a->h * a->w < ((int64_t)1 << 31), "vis_max_preds: map too large");
    int rc = validate_vis_map("vis_max_preds", a->dtype, a->layout);
    if (rc) return rc;
    FPD_REQUIRE((const void*)a->preds != a->hm && (const void*)a->maxvals != a->hm && a->preds != a->maxvals, "vis_max_preds: an output aliases another buffer");
    rc = fpd_vis_max_preds_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_vis_joints_grid(const fpd_vis_joints_grid_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->image && a->minmax && a->joints && a->vis && a->canvas, "vis_joints_grid: null pointer");
    FPD_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->J > 0, "vis_joints_grid: bad dims");
    FPD_REQUIRE(a->nrow >= 1, "vis_joints_grid: nrow = %d (>= 1)", a->nrow);
    FPD_REQUIRE(a->padding >= 0 && a->padding <= 4096, "vis_joints_grid: padding = %d (0..4096)", a->padding);
    FPD_REQUIRE(a->joints_stride >= 2, "vis_joints_grid: joints_stride = %d (>= 2)", a->joints_stride);
    FPD_REQUIRE((int64_t)a->N * 3 * a->H * a->W < ((int64_t)1 << 40), "vis_joints_grid: image too large");
    const int64_t bytes = fpd_vis_joints_canvas_bytes(*a);
    FPD_REQUIRE(bytes < ((int64_t)1 << 31), "vis_joints_grid: canvas too large");
    FPD_REQUIRE(a->canvas_bytes == bytes, "vis_joints_grid: canvas_bytes = %lld, the grid takes %lld", (long long)a->canvas_bytes, (long long)bytes);
    const void* c = a->canvas;
    FPD_REQUIRE(c != (const void*)a->image && c != (const void*)a->minmax && c != a->joints && c != (const void*)a->vis,
                "vis_joints_grid: canvas aliases an input");
    int rc = fpd_vis_joints_grid_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_vis_heatmap_grid(const fpd_vis_heatmap_grid_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->image && a->hm && a->preds && a->table && a->canvas && (a->minmax || !a->normalize), "vis_heatmap_grid: null pointer");
    FPD_REQUIRE(a->N > 0 && a->h > 0 && a->w > 0 && a->J > 0 && a->J <= FPD_MAX_JOINTS, "vis_heatmap_grid: bad dims (J <= %d)", FPD_MAX_JOINTS);
    FPD_REQUIRE(a->H == 4 * a->h && a->W == 4 * a->w, "vis_heatmap_grid: image %dx%d is not 4x the %dx%d heat map", a->H, a->W, a->h, a->w);
    FPD_REQUIRE((int64_t)a->N * a->J * a->h * a->w < ((int64_t)1 << 31), "vis_heatmap_grid: map too large");
    int rc = validate_vis_map("vis_heatmap_grid", a->dtype, a->layout);
    if (rc) return rc;
    const int64_t bytes = (int64_t)a->N * a->h * (a->J + 1) * a->w * 3;
    FPD_REQUIRE(a->canvas_bytes == bytes, "vis_heatmap_grid: canvas_bytes = %lld, the grid takes %lld", (long long)a->canvas_bytes, (long long)bytes);
    const void* c = a->canvas;
    FPD_REQUIRE(c != (const void*)a->image && c != (const void*)a->minmax && c != a->hm && c != (const void*)a->preds && c != (const void*)a->table,
                "vis_heatmap_grid: canvas aliases an input");
    rc = fpd_vis_heatmap_grid_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_render_targets(const fpd_targets_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->joints && a->vis && a->g && a->target && a->weight, "render_targets: null pointer");
    FPD_REQUIRE(a->B > 0 && a->J > 0 && a->H > 0 && a->W > 0 && a->patch > 0 && (a->patch & 1), "render_targets: bad dims");
    FPD_REQUIRE(a->stride_x > 0 && a->stride_y > 0, "render_targets: bad stride");
    int rc = fpd_render_targets_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_warp_affine(const fpd_warp_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->src && a->out, "warp_affine: null pointer");
    FPD_REQUIRE(a->B > 0 && a->B <= 65535 && a->H > 0 && a->W > 0, "warp_affine: bad dims");
    for (int c = 0; c < 3; ++c) FPD_REQUIRE(a->std[c] != 0.f, "warp_affine: std[%d] == 0", c);
    int rc = fpd_warp_affine_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_augment_params(const fpd_augment_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->idx && a->crop && a->trans && a->joints && a->vis && a->center && a->scale && a->rotation && a->flipped,
                "augment_params: null pointer");
    const fpd_aug_db_t& d = a->db;
    FPD_REQUIRE(d.images && d.joints && d.vis && d.center && d.scale && d.flip_src && d.upper, "augment_params: null database pointer");
    FPD_REQUIRE(d.N > 0 && d.J > 0 && d.J <= 64, "augment_params: bad database dims (N=%d, J=%d; J <= 64)", d.N, d.J);
    FPD_REQUIRE(a->B > 0 && a->out_w > 0 && a->out_h > 0 && a->idx_stride > 0, "augment_params: bad dims");
    FPD_REQUIRE(!a->is_train || (a->draws && a->draw_stride >= 6), "augment_params: training mode needs a draw table of >= 6 columns");
    FPD_REQUIRE(d.aspect_ratio > 0 && d.pixel_std > 0 && a->sf >= 0 && a->rf >= 0, "augment_params: bad scalars");
    int rc = fpd_augment_params_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_warp_affine_aug(const fpd_warp_aug_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->images && a->crop && a->out, "warp_affine_aug: null pointer");
    FPD_REQUIRE(a->B > 0 && a->B <= 65535 && a->H > 0 && a->W > 0 && a->N > 0, "warp_affine_aug: bad dims");
    for (int c = 0; c < 3; ++c) FPD_REQUIRE(a->std[c] != 0.f, "warp_affine_aug: std[%d] == 0", c);
    int rc = fpd_warp_affine_aug_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_oks_nms(const fpd_oks_nms_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->offsets && a->n_keep, "oks_nms: null pointer");
    FPD_REQUIRE(a->P_total >= 0 && a->n_img >= 0 && a->grid >= 0, "oks_nms: negative size (P_total=%d, n_img=%d, grid=%d)", a->P_total, a->n_img, a->grid);
    FPD_REQUIRE(a->J >= 1 && a->J <= 64, "oks_nms: J=%d outside 1..64", a->J);
    FPD_REQUIRE((a->soft == 0 || a->soft == 1) && (a->rescore == 0 || a->rescore == 1), "oks_nms: soft / rescore must be 0 or 1");
    FPD_REQUIRE(a->oks_thre == a->oks_thre && a->in_vis_thre == a->in_vis_thre && (!a->soft || a->oks_thre != 0.0), "oks_nms: bad threshold");
    FPD_REQUIRE(a->sigmas, "oks_nms: null pointer (sigmas)");
    FPD_REQUIRE(a->P_total == 0 || (a->kpts && a->area && a->box_score && a->score && a->work && a->keep), "oks_nms: null pointer (per-person array)");
    FPD_REQUIRE((int64_t)a->P_total * a->J * 3 < (1ll << 40), "oks_nms: too many people");
    if (a->n_img == 0) return 0;
    int rc = fpd_oks_nms_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_coco_match(const fpd_coco_match_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->gt_offsets && a->dt_offsets && a->oks_offsets && a->status, "coco_match: null pointer");
    FPD_REQUIRE(a->n_img >= 0 && a->G_total >= 0 && a->D_total >= 0 && a->grid >= 0 && a->oks_total >= 0,
                "coco_match: negative size (n_img=%d, G_total=%d, D_total=%d, grid=%d)", a->n_img, a->G_total, a->D_total, a->grid);
    FPD_REQUIRE(a->J >= 1 && a->J <= 64, "coco_match: J=%d outside 1..64", a->J);
    FPD_REQUIRE(a->sigmas && a->gt_counted, "coco_match: null pointer (sigmas / gt_counted)");
    FPD_REQUIRE(a->G_total == 0 || (a->gt_kpts && a->gt_area && a->gt_bbox && a->gt_flags && a->scratch), "coco_match: null pointer (per-gt array)");
    FPD_REQUIRE(a->D_total == 0 || (a->dt_kpts && a->matched && a->dt_ignored && a->dt_area), "coco_match: null pointer (per-detection array)");
    FPD_REQUIRE(a->oks_total == 0 || a->oks, "coco_match: null pointer (oks)");
    FPD_REQUIRE(a->oks_total <= (int64_t)a->G_total * a->D_total, "coco_match: oks_total exceeds G_total * D_total");
    for (int r = 0; r < FPD_COCO_AREAS; ++r)
        FPD_REQUIRE(a->area_lo[r] < a->area_hi[r], "coco_match: bad area range %d", r);       // (false for a NaN, and for a struct left at zero)
    for (int k = 0; k < FPD_COCO_THRS; ++k)
        FPD_REQUIRE(a->oks_thrs[k] == a->oks_thrs[k], "coco_match: bad threshold %d", k);
    if (a->n_img == 0) return 0;
    int rc = fpd_coco_match_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_coco_accumulate(const fpd_coco_accum_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->npig && a->rec_thrs && a->precision && a->recall && a->status, "coco_accumulate: null pointer");
    FPD_REQUIRE(a->D_total >= 0, "coco_accumulate: negative size (D_total=%d)", a->D_total);
    FPD_REQUIRE(a->n_rec >= 1 && a->n_rec <= 1024, "coco_accumulate: n_rec=%d outside 1..1024", a->n_rec);
    FPD_REQUIRE(a->D_total == 0 || (a->matched && a->dt_ignored && a->order && a->tp && a->env), "coco_accumulate: null pointer (per-detection array)");
    int rc = fpd_coco_accumulate_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_render_targets_w(const fpd_targets_w_t* w, fpd_stream_t stream) {
    FPD_REQUIRE(w, "render_targets_w: null pointer");
    const fpd_targets_t* a = &w->t;
    FPD_REQUIRE(a->joints && a->vis && a->g && a->target && a->weight, "render_targets_w: null pointer");
    FPD_REQUIRE(a->B > 0 && a->J > 0 && a->H > 0 && a->W > 0 && a->patch > 0 && (a->patch & 1), "render_targets_w: bad dims");
    FPD_REQUIRE(a->stride_x > 0 && a->stride_y > 0, "render_targets_w: bad stride");
    int rc = fpd_render_targets_w_launch(*w, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_render_targets_unbiased(const fpd_targets_unbiased_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->joints && a->vis && a->target && a->weight, "render_targets_unbiased: null pointer");
    FPD_REQUIRE(a->B > 0 && a->J > 0 && a->H > 0 && a->W > 0, "render_targets_unbiased: bad dims (B=%d, J=%d, H=%d, W=%d)", a->B, a->J, a->H, a->W);
    FPD_REQUIRE(a->sigma >= 1 && a->sigma <= 4096, "render_targets_unbiased: sigma=%d outside 1..4096", a->sigma);
    FPD_REQUIRE(a->stride_x > 0 && a->stride_y > 0, "render_targets_unbiased: bad stride");
    FPD_REQUIRE((int64_t)a->B * a->J < ((int64_t)1 << 31) && (int64_t)a->H * a->W < ((int64_t)1 << 31), "render_targets_unbiased: map too large");
    FPD_REQUIRE(a->H + a->W <= 8192, "render_targets_unbiased: H + W = %d row and column factors exceed the 64 KB of LDS (8192)", a->H + a->W);
    int rc = fpd_render_targets_unbiased_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_elementwise_pair(const fpd_ew_pair_t* p, fpd_stream_t stream) {
    FPD_REQUIRE(p && p->a.y && p->b.y, "elementwise_pair: null pointer");
    int rc = fpd_elementwise_pair_launch(p->a, p->b, (hipStream_t)stream);
    if (rc == 1) {
        rc = fpd_elementwise_launch(p->a, (hipStream_t)stream);
        if (rc == 0) rc = fpd_elementwise_launch(p->b, (hipStream_t)stream);
    }
    return rc ? rc : check_launch();
}

static int validate_loss_dims(const fpd_loss_t* a, const char* what) {
    FPD_REQUIRE(a, "%s: null pointer", what);
    FPD_REQUIRE(a->B > 0 && a->J > 0 && a->H > 0 && a->W > 0, "%s: non-positive dimension", what);
    if (a->J > FPD_MAX_JOINTS || a->S > FPD_MAX_STACKS || a->S < 1)
        return fpd_fail(-3, "%s: J=%d (<=%d), S=%d (1..%d)", what, a->J, FPD_MAX_JOINTS, a->S, FPD_MAX_STACKS);
    FPD_REQUIRE((int64_t)a->B * a->H * a->W * a->J < ((int64_t)1 << 31), "%s: tensor too large for 32-bit indexing", what);
    return 0;
}

// What every loss entry point asks of its fpd_loss_t, before any launch
static int validate_loss(const fpd_loss_t* a, const char* what) {
    FPD_REQUIRE(a->teacher && a->target && a->weight && a->losses, "%s: null pointer", what);
    const int rc = validate_loss_dims(a, what);
    if (rc) return rc;
    FPD_REQUIRE(a->dtype == FPD_F32 || a->dtype == FPD_BF16, "%s: bad dtype %d", what, a->dtype);
    for (int s = 0; s < a->S; ++s) FPD_REQUIRE(a->out[s], "%s: null map of stack %d", what, s);
    return 0;
}

// The caller's arena of fp64 partial sums against what fpd_<what>_scratch_bytes() answers
static int validate_loss_scratch(const void* scratch, int64_t bytes, int64_t need, const char* what) {
    FPD_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0, "%s: scratch is null or not 8-byte aligned", what);
    FPD_REQUIRE(bytes >= need, "%s: scratch of %lld bytes, fpd_%s_scratch_bytes() asks for %lld", what, (long long)bytes, what, (long long)need);
    return 0;
}

int fpd_loss(const fpd_loss_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a, "loss: null pointer");
    int rc = validate_loss(a, "loss");
    if (rc) return rc;
    rc = fpd_loss_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_loss_geometry(const fpd_loss_t* a, int32_t* vectorised, int32_t* blocks, int32_t* tiles_per_block) {
    FPD_REQUIRE(a && vectorised && blocks && tiles_per_block, "loss_geometry: null pointer");
    FPD_REQUIRE(a->B > 0 && a->J > 0 && a->H > 0 && a->W > 0, "loss_geometry: non-positive dimension");
    int v = 0, b = 0, t = 0;
    const int rc = fpd_loss_geometry_of(*a, &v, &b, &t);
    if (rc) return rc;
    *vectorised = v; *blocks = b; *tiles_per_block = t;
    return 0;
}

int64_t fpd_loss_ohkm_scratch_bytes(const fpd_loss_t* a) {
    const int rc = validate_loss_dims(a, "loss_ohkm_scratch_bytes");
    return rc ? rc : fpd_loss_ohkm_scratch_size(*a);
}

int fpd_loss_ohkm(const fpd_loss_ohkm_t* k, fpd_stream_t stream) {
    FPD_REQUIRE(k, "loss_ohkm: null pointer");
    const fpd_loss_t* a = &k->base;
    int rc = validate_loss(a, "loss_ohkm");
    if (rc) return rc;
    FPD_REQUIRE(k->topk_pose >= 1 && k->topk_pose <= a->J && k->topk_kd >= 1 && k->topk_kd <= a->J,
                "loss_ohkm: topk (%d, %d) outside [1, J=%d]", k->topk_pose, k->topk_kd, a->J);
    rc = validate_loss_scratch(k->scratch, k->scratch_bytes, fpd_loss_ohkm_scratch_size(*a), "loss_ohkm");
    if (rc) return rc;
    rc = fpd_loss_ohkm_launch(*k, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int64_t fpd_loss_kl_scratch_bytes(const fpd_loss_t* a) {
    const int rc = validate_loss_dims(a, "loss_kl_scratch_bytes");
    return rc ? rc : fpd_loss_kl_scratch_size(*a);
}

int fpd_loss_kl(const fpd_loss_kl_t* k, fpd_stream_t stream) {
    FPD_REQUIRE(k, "loss_kl: null pointer");
    const fpd_loss_t* a = &k->base;
    int rc = validate_loss(a, "loss_kl");
    if (rc) return rc;
    FPD_REQUIRE(k->kl_pose || k->kl_kd, "loss_kl: neither term is KL (two MSE terms are fpd_loss)");
    FPD_REQUIRE(!k->kl_pose || (k->temp_pose > 0.f && k->temp_pose < INFINITY), "loss_kl: pose temperature %g is not positive", (double)k->temp_pose);
    FPD_REQUIRE(!k->kl_kd || (k->temp_kd > 0.f && k->temp_kd < INFINITY), "loss_kl: distillation temperature %g is not positive", (double)k->temp_kd);
    rc = validate_loss_scratch(k->scratch, k->scratch_bytes, fpd_loss_kl_scratch_size(*a), "loss_kl");
    if (rc) return rc;
    fpd_loss_kl_t kk = *k;
    if (!kk.kl_pose) kk.temp_pose = 1.f;         // (an MSE term's temperature is not read; keep its reciprocal finite)
    if (!kk.kl_kd) kk.temp_kd = 1.f;
    rc = fpd_loss_kl_launch(kk, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_adam(const fpd_adam_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->param && a->grad && a->m && a->v && a->n >= 0, "adam: null pointer");
    int rc = fpd_adam_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_adamw(const fpd_adamw_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a, "adamw: null pointer");
    int rc = fpd_adamw_launch(*a, (hipStream_t)stream);      // (validates through fpd_adamw_geometry_of before it launches)
    return rc ? rc : check_launch();
}
int fpd_adamw_geometry(const fpd_adamw_t* a, int32_t* blocks, int64_t* vec_elems) {
    FPD_REQUIRE(a && blocks && vec_elems, "adamw_geometry: null pointer");
    int b = 0;
    int64_t nvec = 0;
    const int rc = fpd_adamw_geometry_of(*a, &b, &nvec);
    if (rc) return rc;
    *blocks = b;
    *vec_elems = 4 * nvec;
    return 0;
}

int fpd_sgd(const fpd_sgd_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a && a->param && a->grad, "sgd: null pointer");
    FPD_REQUIRE(a->n >= 0, "sgd: n = %lld is negative", (long long)a->n);
    FPD_REQUIRE(a->momentum >= 0.f, "sgd: invalid momentum value %g", (double)a->momentum);
    FPD_REQUIRE(a->weight_decay >= 0.f, "sgd: invalid weight_decay value %g", (double)a->weight_decay);
    FPD_REQUIRE(a->momentum == 0.f || a->buf, "sgd: momentum %g needs a momentum buffer (buf is null)", (double)a->momentum);
    FPD_REQUIRE(!a->nesterov || a->momentum != 0.f, "sgd: nesterov momentum requires a momentum (and zero dampening)");
    int rc = fpd_sgd_launch(*a, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

int fpd_ema(const fpd_ema_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a, "ema: null pointer");
    int rc = fpd_ema_launch(*a, (hipStream_t)stream);      // (validates through fpd_ema_geometry_of before it launches)
    return rc ? rc : check_launch();
}
int fpd_ema_geometry(const fpd_ema_t* a, int32_t* blocks, int64_t* vec_elems) {
    FPD_REQUIRE(a && blocks && vec_elems, "ema_geometry: null pointer");
    int b = 0;
    int64_t nvec[FPD_EMA_MAX_SEG] = {};
    const int rc = fpd_ema_geometry_of(*a, &b, nvec);
    if (rc) return rc;
    *blocks = b;
    for (int s = 0; s < a->nseg; ++s) vec_elems[s] = 4 * nvec[s];
    return 0;
}

int fpd_grad_clip(const fpd_grad_clip_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a, "grad_clip: null pointer");
    int rc = fpd_grad_clip_launch(*a, (hipStream_t)stream);      // (validates through fpd_grad_clip_geometry_of before it launches)
    return rc ? rc : check_launch();
}
int64_t fpd_grad_clip_scratch_bytes(int64_t n) { return fpd_grad_clip_scratch_size(n); }
int fpd_grad_clip_geometry(const fpd_grad_clip_t* a, int32_t* blocks, int64_t* vec_elems) {
    FPD_REQUIRE(a && blocks && vec_elems, "grad_clip_geometry: null pointer");
    int b = 0;
    int64_t nvec = 0;
    const int rc = fpd_grad_clip_geometry_of(*a, &b, &nvec);
    if (rc) return rc;
    *blocks = b;
    *vec_elems = 4 * nvec;
    return 0;
}

int fpd_grad_accum(const fpd_grad_accum_t* a, fpd_stream_t stream) {
    FPD_REQUIRE(a, "grad_accum: null pointer");
    int rc = fpd_grad_accum_launch(*a, (hipStream_t)stream);      // (validates through fpd_grad_accum_geometry_of before it launches)
    return rc ? rc : check_launch();
}
int fpd_grad_accum_geometry(const fpd_grad_accum_t* a, int32_t* blocks, int64_t* vec_elems) {
    FPD_REQUIRE(a && blocks && vec_elems, "grad_accum_geometry: null pointer");
    int b = 0;
    int64_t nvec = 0;
    const int rc = fpd_grad_accum_geometry_of(*a, &b, &nvec);
    if (rc) return rc;
    *blocks = b;
    *vec_elems = 4 * nvec;
    return 0;
}

int fpd_weight_prep(const fpd_wprep_entry_t* t, int32_t n, int64_t max_elems, int32_t dtype, fpd_stream_t stream) {
    int rc = fpd_weight_prep_launch(t, n, max_elems, dtype, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_bn_update_running(const fpd_bnupd_entry_t* t, int32_t n, fpd_stream_t stream) {
    int rc = fpd_bn_update_running_launch(t, n, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_cast(const void* src, void* dst, int64_t n, int32_t sd, int32_t dd, fpd_stream_t stream) {
    int rc = fpd_cast_launch(src, dst, n, sd, dd, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_nchw_to_nhwc(const float* src, void* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t dtype, fpd_stream_t stream) {
    int rc = fpd_nchw_to_nhwc_launch(src, dst, N, C, H, W, dtype, (hipStream_t)stream);
    return rc ? rc : check_launch();
}
int fpd_nhwc_to_nchw(const void* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t dtype, fpd_stream_t stream) {
    int rc = fpd_nhwc_to_nchw_launch(src, dst, N, C, H, W, dtype, (hipStream_t)stream);
    return rc ? rc : check_launch();
}

// ------------------------------------------------------------------------------------------
// execution plan
// ------------------------------------------------------------------------------------------
struct fpd_op {
    int32_t type;
    union {
        fpd_affsum_t affsum; fpd_layout_t layout; fpd_conv_f8_t conv8; fpd_conv_t conv; fpd_conv_pair_t pair; fpd_bneck_t bneck; fpd_bneck_pair_t bpair; fpd_ew_pair_t epair; fpd_pck_t pck; fpd_head_t head; fpd_wgrad_t wgrad; fpd_stem_t stem; fpd_ew_t ew; fpd_loss_t loss; fpd_loss_ohkm_t lossk; fpd_loss_kl_t losskl; fpd_adam_t adam; fpd_sgd_t sgd; fpd_ew_merge_t ewm; fpd_ema_t ema; fpd_grad_clip_t clip; fpd_grad_accum_t accum; fpd_adamw_t adamw;
        fpd_memset_t mset; fpd_table_t table;
    } u;
};
struct fpd_sched {                       // per-op multi-lane schedule (fpd_plan_set_schedule)
    int32_t lane = 0;
    bool record = false;                 // some op of another lane waits for this one
    hipEvent_t done = nullptr;
    std::vector<int32_t> waits;
};
struct fpd_plan {
    std::vector<fpd_op> ops;
    std::vector<fpd_sched> sched;
    std::vector<hipGraphExec_t> graphs;
    std::vector<hipGraph_t> graph_defs;
    hipStream_t lanes[FPD_MAX_LANES] = {};      // [0] unused: lane 0 is the caller's stream
    hipEvent_t lane_done[FPD_MAX_LANES] = {};
    hipEvent_t fork = nullptr;
};

fpd_plan* fpd_plan_create(void) { return new fpd_plan(); }
void fpd_plan_destroy(fpd_plan* p) {
    if (!p) return;
    for (auto g : p->graphs) (void)hipGraphExecDestroy(g);
    for (auto g : p->graph_defs) (void)hipGraphDestroy(g);
    for (auto& s : p->sched) if (s.done) (void)hipEventDestroy(s.done);
    for (int l = 0; l < FPD_MAX_LANES; ++l) {
        if (p->lanes[l]) (void)hipStreamDestroy(p->lanes[l]);
        if (p->lane_done[l]) (void)hipEventDestroy(p->lane_done[l]);
    }
    if (p->fork) (void)hipEventDestroy(p->fork);
    delete p;
}
int fpd_plan_size(const fpd_plan* p) { return p ? (int)p->ops.size() : -1; }

int fpd_plan_add(fpd_plan* p, int32_t op, const void* args, int64_t bytes) {
    FPD_REQUIRE(p && args, "plan_add: null");
    fpd_op o;
    memset(&o, 0, sizeof(o));
    o.type = op;
    size_t want = 0;
    switch (op) {
        case FPD_OP_CONV: want = sizeof(fpd_conv_t); break;
        case FPD_OP_CONV_F8: want = sizeof(fpd_conv_f8_t); break;
        case FPD_OP_WGRAD: want = sizeof(fpd_wgrad_t); break;
        case FPD_OP_CONV_PAIR: want = sizeof(fpd_conv_pair_t); break;
        case FPD_OP_BNECK_PAIR: want = sizeof(fpd_bneck_pair_t); break;
        case FPD_OP_EW_PAIR: want = sizeof(fpd_ew_pair_t); break;
        case FPD_OP_PCK: want = sizeof(fpd_pck_t); break;
        case FPD_OP_HEAD: case FPD_OP_HEAD_FOLD: want = sizeof(fpd_head_t); break;
        case FPD_OP_BNECK: case FPD_OP_BNECK_FOLD: want = sizeof(fpd_bneck_t); break;
        case FPD_OP_STEM_FWD: case FPD_OP_STEM_WGRAD: want = sizeof(fpd_stem_t); break;
        case FPD_OP_EW: want = sizeof(fpd_ew_t); break;
        case FPD_OP_EW_MERGE: want = sizeof(fpd_ew_merge_t); break;
        case FPD_OP_LOSS: want = sizeof(fpd_loss_t); break;
        case FPD_OP_LOSS_OHKM: want = sizeof(fpd_loss_ohkm_t); break;
        case FPD_OP_LOSS_KL: want = sizeof(fpd_loss_kl_t); break;
        case FPD_OP_ADAM: want = sizeof(fpd_adam_t); break;
        case FPD_OP_ADAMW: want = sizeof(fpd_adamw_t); break;
        case FPD_OP_SGD: want = sizeof(fpd_sgd_t); break;
        case FPD_OP_EMA: want = sizeof(fpd_ema_t); break;
        case FPD_OP_GRAD_CLIP: want = sizeof(fpd_grad_clip_t); break;
        case FPD_OP_GRAD_ACCUM: want = sizeof(fpd_grad_accum_t); break;
        case FPD_OP_MEMSET: case FPD_OP_NOP: want = sizeof(fpd_memset_t); break;
        case FPD_OP_AFFSUM: want = sizeof(fpd_affsum_t); break;
        case FPD_OP_NCHW2NHWC: want = sizeof(fpd_layout_t); break;
        case FPD_OP_WPREP: case FPD_OP_BNUPD: case FPD_OP_WREDUCE: case FPD_OP_WQUANT: want = sizeof(fpd_table_t); break;
        default: return fpd_fail(-2, "plan_add: unknown op %d", op);
    }
    FPD_REQUIRE((size_t)bytes == want, "plan_add: op %d expects %zu bytes of args, got %lld", op, want, (long long)bytes);
    memcpy(&o.u, args, want);
    p->ops.push_back(o);
    p->sched.emplace_back();
    return (int)p->ops.size() - 1;
}

int fpd_plan_set_schedule(fpd_plan* p, int32_t op, int32_t lane, const int32_t* wait_ops, int32_t n_waits) {
    FPD_REQUIRE(p && op >= 0 && op < (int)p->ops.size(), "plan_set_schedule: bad op index %d", op);
    FPD_REQUIRE(lane >= 0 && lane < FPD_MAX_LANES, "plan_set_schedule: lane %d outside [0,%d)", lane, FPD_MAX_LANES);
    FPD_REQUIRE(n_waits >= 0 && (n_waits == 0 || wait_ops != nullptr), "plan_set_schedule: bad wait list");
    for (int i = 0; i < n_waits; ++i)
        FPD_REQUIRE(wait_ops[i] >= 0 && wait_ops[i] < op, "plan_set_schedule: op %d may only wait for earlier ops (got %d)", op, wait_ops[i]);
    fpd_sched& s = p->sched[op];
    s.lane = lane;
    s.waits.assign(wait_ops, wait_ops + n_waits);
    for (int i = 0; i < n_waits; ++i) p->sched[wait_ops[i]].record = true;
    return 0;
}

int fpd_plan_mark_event(fpd_plan* p, int32_t op) {
    FPD_REQUIRE(p && op >= 0 && op < (int)p->ops.size(), "plan_mark_event: bad op index %d", op);
    p->sched[op].record = true;
    return 0;
}

int fpd_plan_wait_op(fpd_plan* p, int32_t op, fpd_stream_t stream) {
    FPD_REQUIRE(p && op >= 0 && op < (int)p->ops.size(), "plan_wait_op: bad op index %d", op);
    FPD_REQUIRE(p->sched[op].record && p->sched[op].done, "plan_wait_op: op %d has no recorded event (mark it, then run its range)", op);
    FPD_CHECK_HIP(hipStreamWaitEvent((hipStream_t)stream, p->sched[op].done, 0));
    return 0;
}

static void conv_tag(char* p, size_t n, const char* what, const fpd_conv_t& c) {
    snprintf(p, n, "%s N=%d H=%d W=%d C=%d K=%d R=%d s=%d %s%s%s%s%s", what, c.N, c.H, c.W, c.C, c.K, c.R, c.stride,
             c.epi == FPD_EPI_BNRELU_BWD ? "dgrad" : "fwd", c.bn.mode == FPD_BN_EVAL ? " evalbn" : "", c.wg_partial ? " +wgrad" : "", c.fold_x ? " +fold" : "",
             c.x2 ? " +skip" : "");
}
// "<plan op index> <what> <shape>": the key tools/profile_summarize.py groups trace rows by
static void set_op_tag(int idx, const fpd_op& o) {
    char t[200] = "";
    static const char* ew_names[] = {"bnrelu_fwd", "bnrelu_bwd_r", "bn_bwd_apply", "maxpool_fwd", "maxpool_bwd", "upadd_fwd", "sumpool", "add", "relu_mask", "dilate2"};
    auto ewn = [&](int op) { return (op >= 0 && op < 10) ? ew_names[op] : "ew"; };
    switch (o.type) {
        case FPD_OP_CONV: conv_tag(t, sizeof(t), "conv", o.u.conv); break;
        case FPD_OP_CONV_F8: conv_tag(t, sizeof(t), "conv_f8", o.u.conv8.c); break;
        case FPD_OP_CONV_PAIR: {
            char a[90], b[90];
            conv_tag(a, sizeof(a), "conv2", o.u.pair.a);
            snprintf(b, sizeof(b), " | H=%d W=%d", o.u.pair.b.H, o.u.pair.b.W);
            snprintf(t, sizeof(t), "%s%s", a, b);
            break;
        }
        case FPD_OP_WGRAD: snprintf(t, sizeof(t), "wgrad N=%d H=%d W=%d C=%d K=%d R=%d s=%d", o.u.wgrad.N, o.u.wgrad.H, o.u.wgrad.W, o.u.wgrad.C, o.u.wgrad.K, o.u.wgrad.R, o.u.wgrad.stride); break;
        case FPD_OP_BNECK: snprintf(t, sizeof(t), "bneck N=%d H=%d W=%d C=%d P=%d%s", o.u.bneck.N, o.u.bneck.H, o.u.bneck.W, o.u.bneck.C, o.u.bneck.P, o.u.bneck.x2 ? "+upadd" : ""); break;
        case FPD_OP_BNECK_PAIR: snprintf(t, sizeof(t), "bneck2 N=%d H=%d W=%d C=%d P=%d | H=%d W=%d", o.u.bpair.a.N, o.u.bpair.a.H, o.u.bpair.a.W, o.u.bpair.a.C, o.u.bpair.a.P, o.u.bpair.b.H, o.u.bpair.b.W); break;
        case FPD_OP_HEAD: snprintf(t, sizeof(t), "head N=%d H=%d W=%d C=%d J=%d", o.u.head.N, o.u.head.H, o.u.head.W, o.u.head.C, o.u.head.J); break;
        case FPD_OP_EW: snprintf(t, sizeof(t), "ew %s N=%d H=%d W=%d C=%d", ewn(o.u.ew.op), o.u.ew.N, o.u.ew.H, o.u.ew.W, o.u.ew.C); break;
        case FPD_OP_EW_PAIR: snprintf(t, sizeof(t), "ew2 %s N=%d H=%d W=%d C=%d | H=%d W=%d", ewn(o.u.epair.a.op), o.u.epair.a.N, o.u.epair.a.H, o.u.epair.a.W, o.u.epair.a.C, o.u.epair.b.H, o.u.epair.b.W); break;
        case FPD_OP_EW_MERGE: {
            const fpd_ew_merge_t& m = o.u.ewm;
            const bool pb = m.kind == FPD_EWM_MAXPOOL_BWD;
            snprintf(t, sizeof(t), "ewm %s N=%d H=%d W=%d C=%d", pb ? (m.has_full ? "apply2+maxpool_bwd" : "apply+maxpool_bwd") : "apply+sumpool", m.pool.N, m.pool.H, m.pool.W, m.pool.C);
            break;
        }
        case FPD_OP_STEM_FWD: case FPD_OP_STEM_WGRAD: snprintf(t, sizeof(t), "%s N=%d H=%d W=%d K=%d%s", o.type == FPD_OP_STEM_FWD ? "stem_fwd" : "stem_wgrad", o.u.stem.N, o.u.stem.H, o.u.stem.W, o.u.stem.K,
                                                              (o.type == FPD_OP_STEM_FWD && o.u.stem.act.mode != FPD_BN_NONE) ? " +act" : ""); break;
        case FPD_OP_AFFSUM: snprintf(t, sizeof(t), "affsum N=%d H=%d W=%d C=%d terms=%d", o.u.affsum.N, o.u.affsum.H, o.u.affsum.W, o.u.affsum.C, o.u.affsum.nterms); break;
        case FPD_OP_LOSS: snprintf(t, sizeof(t), "loss B=%d J=%d H=%d W=%d S=%d", o.u.loss.B, o.u.loss.J, o.u.loss.H, o.u.loss.W, o.u.loss.S); break;
        case FPD_OP_LOSS_OHKM: snprintf(t, sizeof(t), "loss_ohkm B=%d J=%d H=%d W=%d S=%d k=%d,%d", o.u.lossk.base.B, o.u.lossk.base.J, o.u.lossk.base.H, o.u.lossk.base.W, o.u.lossk.base.S, o.u.lossk.topk_pose, o.u.lossk.topk_kd); break;
        case FPD_OP_LOSS_KL: snprintf(t, sizeof(t), "loss_kl B=%d J=%d H=%d W=%d S=%d kl=%d,%d T=%g,%g", o.u.losskl.base.B, o.u.losskl.base.J, o.u.losskl.base.H, o.u.losskl.base.W, o.u.losskl.base.S, o.u.losskl.kl_pose, o.u.losskl.kl_kd, (double)o.u.losskl.temp_pose, (double)o.u.losskl.temp_kd); break;
        case FPD_OP_ADAM: snprintf(t, sizeof(t), "adam n=%lld", (long long)o.u.adam.n); break;
        case FPD_OP_ADAMW: snprintf(t, sizeof(t), "adamw n=%lld wd=%g%s%s", (long long)o.u.adamw.n, (double)o.u.adamw.weight_decay, o.u.adamw.vmax ? " amsgrad" : "", o.u.adamw.no_decay_bits ? " mask" : ""); break;
        case FPD_OP_SGD: snprintf(t, sizeof(t), "sgd n=%lld momentum=%g wd=%g%s", (long long)o.u.sgd.n, (double)o.u.sgd.momentum, (double)o.u.sgd.weight_decay, o.u.sgd.nesterov ? " nesterov" : ""); break;
        case FPD_OP_EMA: snprintf(t, sizeof(t), "ema nseg=%d n0=%lld decay=%g%s", o.u.ema.nseg, (long long)o.u.ema.seg[0].n, o.u.ema.decay, o.u.ema.warmup ? " warmup" : ""); break;
        case FPD_OP_GRAD_CLIP: snprintf(t, sizeof(t), "grad_clip n=%lld max_norm=%g", (long long)o.u.clip.n, (double)o.u.clip.max_norm); break;
        case FPD_OP_GRAD_ACCUM: snprintf(t, sizeof(t), "grad_accum n=%lld mode=%d", (long long)o.u.accum.n, o.u.accum.mode); break;
        case FPD_OP_WREDUCE: snprintf(t, sizeof(t), "wreduce entries=%d", o.u.table.n); break;
        case FPD_OP_WPREP: snprintf(t, sizeof(t), "wprep entries=%d", o.u.table.n); break;
        case FPD_OP_BNUPD: snprintf(t, sizeof(t), "bnupd entries=%d", o.u.table.n); break;
        default: snprintf(t, sizeof(t), "op%d", o.type); break;
    }
    snprintf(g_op_tag, sizeof(g_op_tag), "%d\t%s", idx, t);
}

static int run_op(const fpd_op& o, fpd_stream_t s) {
    switch (o.type) {
        case FPD_OP_CONV: return fpd_conv_forward(&o.u.conv, s);
        case FPD_OP_CONV_F8: return fpd_conv_forward_f8(&o.u.conv8, s);
        case FPD_OP_WQUANT: return fpd_weight_quant_f8((const fpd_wquant_entry_t*)o.u.table.table, o.u.table.n, s);
        case FPD_OP_WGRAD: return fpd_conv_wgrad(&o.u.wgrad, s);
        case FPD_OP_CONV_PAIR: return fpd_conv_forward_pair(&o.u.pair, s);
        case FPD_OP_BNECK_PAIR: return fpd_bottleneck_forward_pair(&o.u.bpair, s);
        case FPD_OP_EW_PAIR: return fpd_elementwise_pair(&o.u.epair, s);
        case FPD_OP_PCK: return fpd_pck(&o.u.pck, s);
        case FPD_OP_HEAD: return fpd_head_forward(&o.u.head, s);
        case FPD_OP_HEAD_FOLD: return fpd_head_fold(&o.u.head, s);
        case FPD_OP_BNECK: return fpd_bottleneck_forward(&o.u.bneck, s);
        case FPD_OP_BNECK_FOLD: return fpd_bottleneck_fold(&o.u.bneck, s);
        case FPD_OP_STEM_FWD: return fpd_stem_forward(&o.u.stem, s);
        case FPD_OP_STEM_WGRAD: return fpd_stem_wgrad(&o.u.stem, s);
        case FPD_OP_EW: return fpd_elementwise(&o.u.ew, s);
        case FPD_OP_EW_MERGE: return fpd_ew_merge(&o.u.ewm, s);
        case FPD_OP_LOSS: return fpd_loss(&o.u.loss, s);
        case FPD_OP_LOSS_OHKM: return fpd_loss_ohkm(&o.u.lossk, s);
        case FPD_OP_LOSS_KL: return fpd_loss_kl(&o.u.losskl, s);
        case FPD_OP_ADAM: return fpd_adam(&o.u.adam, s);
        case FPD_OP_ADAMW: return fpd_adamw(&o.u.adamw, s);
        case FPD_OP_SGD: return fpd_sgd(&o.u.sgd, s);
        case FPD_OP_EMA: return fpd_ema(&o.u.ema, s);
        case FPD_OP_GRAD_CLIP: return fpd_grad_clip(&o.u.clip, s);
        case FPD_OP_GRAD_ACCUM: return fpd_grad_accum(&o.u.accum, s);
        case FPD_OP_MEMSET: {
            FPD_CHECK_HIP(hipMemsetAsync(o.u.mset.ptr, 0, (size_t)o.u.mset.bytes, (hipStream_t)s));
            return 0;
        }
        case FPD_OP_NOP: return 0;
        case FPD_OP_AFFSUM: return fpd_affsum(&o.u.affsum, s);
        case FPD_OP_NCHW2NHWC:
            return fpd_nchw_to_nhwc(o.u.layout.src, o.u.layout.dst, o.u.layout.N, o.u.layout.C, o.u.layout.H, o.u.layout.W, o.u.layout.dtype, s);
        case FPD_OP_WPREP:
            return fpd_weight_prep((const fpd_wprep_entry_t*)o.u.table.table, o.u.table.n, o.u.table.max_elems, o.u.table.dtype, s);
        case FPD_OP_BNUPD: return fpd_bn_update_running((const fpd_bnupd_entry_t*)o.u.table.table, o.u.table.n, s);
        case FPD_OP_WREDUCE: return fpd_wgrad_reduce((const fpd_wreduce_entry_t*)o.u.table.table, o.u.table.n, o.u.table.max_elems, s);
    }
    return fpd_fail(-2, "run_op: unknown op %d", o.type);
}

static int lane_priority() { return 0; }      // side-lane streams at the default priority (stream priorities measured as a no-op eagerly, rounds 1-2; knob removed in round 6)

static int side_streams() { return FPD_MAX_LANES; }      // one physical stream per lane (the FPD_SIDE_STREAMS knob of rounds 1-5 never beat it)

int fpd_plan_run(fpd_plan* p, int32_t begin, int32_t end, fpd_stream_t stream) {
    FPD_REQUIRE(p && begin >= 0 && end <= (int)p->ops.size() && begin <= end, "plan_run: bad range [%d,%d)", begin, end);
    hipStream_t main_s = (hipStream_t)stream;
    bool multi = false;
    for (int i = begin; i < end; ++i) multi |= p->sched[i].lane != 0;
    bool used[FPD_MAX_LANES] = {};
    if (multi) {
        if (!p->fork) FPD_CHECK_HIP(hipEventCreateWithFlags(&p->fork, hipEventDisableTiming));
        FPD_CHECK_HIP(hipEventRecord(p->fork, main_s));
    }
    int rc = 0;
    for (int i = begin; i < end && rc == 0; ++i) {
        fpd_sched& sc = p->sched[i];
        hipStream_t st = main_s;
        if (sc.lane != 0) {
            const int l = 1 + (sc.lane - 1) % side_streams();
            if (!p->lanes[l]) {
                FPD_CHECK_HIP(hipStreamCreateWithPriority(&p->lanes[l], hipStreamNonBlocking, lane_priority()));
                FPD_CHECK_HIP(hipEventCreateWithFlags(&p->lane_done[l], hipEventDisableTiming));
            }
            st = p->lanes[l];
            if (!used[l]) {                      // fork: the lane starts after everything already queued on `stream`
                FPD_CHECK_HIP(hipStreamWaitEvent(st, p->fork, 0));
                used[l] = true;
            }
        }
        for (int32_t w : sc.waits)
            if (w >= begin && w < end) FPD_CHECK_HIP(hipStreamWaitEvent(st, p->sched[w].done, 0));
        if (g_fpd_launch_log) set_op_tag(i, p->ops[i]);
        rc = run_op(p->ops[i], (fpd_stream_t)st);
        if (rc) {
            char tmp[400];
            snprintf(tmp, sizeof(tmp), "%s", g_err);
            rc = fpd_fail(rc, "plan op %d (type %d): %s", i, p->ops[i].type, tmp);
            break;
        }
        if (sc.record) {
            if (!sc.done) FPD_CHECK_HIP(hipEventCreateWithFlags(&sc.done, hipEventDisableTiming));
            FPD_CHECK_HIP(hipEventRecord(sc.done, st));
        }
    }
    // join (also on failure, so that a stream capture in progress can be closed cleanly)
    for (int l = 1; l < FPD_MAX_LANES; ++l)
        if (used[l]) {
            FPD_CHECK_HIP(hipEventRecord(p->lane_done[l], p->lanes[l]));
            FPD_CHECK_HIP(hipStreamWaitEvent(main_s, p->lane_done[l], 0));
        }
    return rc;
}

int fpd_plan_run_op(fpd_plan* p, int32_t op, fpd_stream_t stream) {
    FPD_REQUIRE(p && op >= 0 && op < (int)p->ops.size(), "plan_run_op: bad op index %d", op);
    if (g_fpd_launch_log) set_op_tag(op, p->ops[op]);
    return run_op(p->ops[op], stream);
}

int fpd_plan_capture(fpd_plan* p, int32_t begin, int32_t end, fpd_stream_t stream) {
    FPD_REQUIRE(p, "plan_capture: null");
    // a captured launch is logged once (here) but traced on every replay: the log could no longer be aligned with a trace
    FPD_REQUIRE(!g_fpd_launch_log, "plan_capture: FPD_LAUNCH_LOG is set -- the launch log keys a kernel trace 1:1 and cannot follow hipGraph replays; unset one of them");
    hipStream_t st = (hipStream_t)stream;
    FPD_CHECK_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = fpd_plan_run(p, begin, end, stream);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(st, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return fpd_fail(-100 - (int)e, "hipStreamEndCapture: %s", hipGetErrorString(e));
    hipGraphExec_t ge = nullptr;
    FPD_CHECK_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    p->graph_defs.push_back(g);
    p->graphs.push_back(ge);
    return (int)p->graphs.size() - 1;
}

int fpd_plan_replay(fpd_plan* p, int32_t gid, fpd_stream_t stream) {
    FPD_REQUIRE(p && gid >= 0 && gid < (int)p->graphs.size(), "plan_replay: bad graph id %d", gid);
    FPD_CHECK_HIP(hipGraphLaunch(p->graphs[gid], (hipStream_t)stream));
    return 0;
}

void* fpd_event_create(void) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return (void*)e;
}
int fpd_event_record(void* ev, fpd_stream_t stream) {
    FPD_CHECK_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return 0;
}
float fpd_event_elapsed_ms(void* start, void* stop) {
    float ms = -1.f;
    if (hipEventSynchronize((hipEvent_t)stop) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, (hipEvent_t)start, (hipEvent_t)stop) != hipSuccess) return -1.f;
    return ms;
}
void fpd_event_destroy(void* ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }

}  // extern "C"
