// Internal entry points of the kernel units, as api.hip dispatches to them (host code only).
//
// Launch convention: 0 = launched, 1 = outside this kernel's domain (the caller tries the next one), < 0 error.
#pragma once
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdlib>

#include "common.h"

// An integer option of a kernel unit: its environment variable is read once, at the first use; fpd_set_option (the units'
// *_option entry points) overrides it at run time and gets the previous value back.  A value below 0 means "not read yet".
struct EnvOpt {
    const char* env; int def, lo = INT_MIN, v = -1;       // variable, default, smallest value get() returns
    int get() { if (v < 0) { const char* e = getenv(env); v = e ? atoi(e) : def; } return v < lo ? lo : v; }
    int set(int value) { const int prev = get(); v = value; return prev; }
};

// The grid cap of a persistent kernel (the fused teacher kernels: below the CU count, so that the streams running next to them find
// free compute units).  The environment supplies the default, raised to at least 8; fpd_set_option (the units' *_blocks_option entry
// points) takes any n >= 1 -- tests let one block walk many tiles of a small tensor -- and gets the value in force back.  0 = not set
// yet: a value set before the first launch wins over the environment.
struct GridCap {
    const char* env; int def;
    std::atomic<int> v{0};
    int get() {
        int cap = v.load(std::memory_order_relaxed);
        if (!cap) {
            const char* e = getenv(env);
            cap = std::max(8, e ? atoi(e) : def);
            int unset = 0;                 // (a value set through fpd_set_option in the meantime wins)
            if (!v.compare_exchange_strong(unset, cap, std::memory_order_relaxed)) cap = unset;
        }
        return cap;
    }
    int set(int value) { get(); return v.exchange(std::max(1, value), std::memory_order_relaxed); }
};

// Persistent blocks for `units` work units (tiles, rounds, strips) under a cap, balanced: every block walks the same number of them --
// 512 rounds under a cap of 192 -> 171 blocks of 3, not 192 blocks of which two thirds run 3 and the rest 2.
inline int fpd_balanced_blocks(int units, int cap) { return units <= cap ? units : cdiv(units, cdiv(units, cap)); }

// The blocks of a streaming launch.  A pair launch (ub > 0 units of a second convolution) shares them in proportion, at least one
// each; false: a pair with a single block.
inline bool fpd_split_blocks(int ua, int ub, bool pair, int cap, int& na, int& nb) {
    const int total = fpd_balanced_blocks(ua + ub, std::max(1, cap));
    nb = 0;
    if (pair) {
        if (total < 2) return false;
        nb = std::max(1, std::min(total - 1, (int)((long long)total * ub / (ua + ub))));
    }
    na = total - nb;
    return true;
}

// ---- convolutions: conv_c1 / conv_c3 / conv_pp / conv_tile decide in ONE route function each, which their launch and the
//      queries of api.hip (fold, slab count) both go through ----
// What the launch (b != nullptr: the pair launch) WILL carry, whatever the descriptor fields hold now: the queries are asked
// before the caller fills in the fold and slab fields.
// (skip: the launch carries a second 1x1 source, fpd_conv_t.x2 -- only conv_c1 offers it, every other route declines such a launch)
struct ConvAsk { bool fold, wg, skip; };   // some convolution of the launch folds a BN-backward apply / forms a weight gradient / has a second source
struct ConvRoute { bool folds; int slabs_a, slabs_b; bool skips; };      // the fold is evaluated; weight-gradient slabs written for a / b (0: none); the second source is formed
inline ConvAsk fpd_conv_ask(const fpd_conv_t& a, const fpd_conv_t* b) {
    return ConvAsk{a.fold_x != nullptr || (b != nullptr && b->fold_x != nullptr), a.wg_partial != nullptr || (b != nullptr && b->wg_partial != nullptr),
                   a.x2 != nullptr || (b != nullptr && b->x2 != nullptr)};
}
// the slab fields of a launch against the slab count of its route (the count was asked for when the workspace was sized; a
// geometry that has changed since would write past the workspace or leave slabs unwritten)
inline int fpd_conv_check_slabs(const fpd_conv_t& c, int slabs, const char* unit) {
    if (c.wg_partial == nullptr) return 0;
    FPD_REQUIRE(c.wg_stride >= (int64_t)c.C * c.K + c.C, "conv: wg_stride %lld smaller than weight + bias", (long long)c.wg_stride);
    FPD_REQUIRE(c.wg_count == slabs, "conv: the launch writes %d weight-gradient slabs but the caller sized its workspace for %d "
                "(fpd_conv_fused_wgrad_partials: has a %s option changed since?)", slabs, c.wg_count, unit);
    return 0;
}
// route: 0 = this kernel takes the launch carrying `ask` (r: what it offers), 1 = it declines.  launch: routes with the ask read
// from the fields, then launches.
int fpd_conv_c1_route(const fpd_conv_t& a, const fpd_conv_t* b, ConvAsk ask, ConvRoute& r);
int fpd_conv_c1_launch(const fpd_conv_t& a, const fpd_conv_t* b, hipStream_t st);
int fpd_conv_c3_route(const fpd_conv_t& a, const fpd_conv_t* b, ConvAsk ask, ConvRoute& r);
int fpd_conv_c3_launch(const fpd_conv_t& a, const fpd_conv_t* b, hipStream_t st);
int fpd_conv_pp_route(const fpd_conv_t& a, const fpd_conv_t* b, ConvAsk ask, ConvRoute& r);
int fpd_conv_pp_launch(const fpd_conv_t& a, const fpd_conv_t* b, hipStream_t st);
int fpd_conv_tile_route(const fpd_conv_t& a, const fpd_conv_t* b, ConvAsk ask, ConvRoute& r);
int fpd_conv_tile_launch(const fpd_conv_t& a, const fpd_conv_t* b, hipStream_t st);
int fpd_conv_tile_variant_of(const fpd_conv_t& a, const fpd_conv_t* b, ConvAsk ask);      // the instantiation that launch runs (packed, see conv_tile.hip), -1: declined
int fpd_conv_tile_launches();                      // "conv_tile_launches"
int fpd_conv_c1_option(int which, int value);
int fpd_conv_c3_option(int which, int value);
int fpd_conv_pp_option(int which, int value);
// the generic kernels and the fp8 tile kernel decide inside their launch: no fold, no fused weight gradient, no pairs
int fpd_conv_mfma_launch(const fpd_conv_t& a, hipStream_t st);
int fpd_conv_smallc_launch(const fpd_conv_t& a, hipStream_t st);
int fpd_conv_naive_launch(const fpd_conv_t& a, hipStream_t st);
bool fpd_conv_f8_domain(const fpd_conv_t& a);
int fpd_conv_f8_variant_of(const fpd_conv_t& a);          // the conv_tile_f8_kernel instantiation the launch runs: TN | BK << 4, -1: declined
int fpd_conv_tile_f8_launch(const fpd_conv_t& a, const void* w8, const float* wscale, hipStream_t st);
int fpd_weight_quant_f8_launch(const fpd_wquant_entry_t* table, int n, hipStream_t st);

// ---- weight gradients: *_partials = slabs the launch of the same unit writes (0: it declines) ----
int fpd_wgrad_tile_partials(const fpd_wgrad_t& a);
int fpd_wgrad_tile_launch(const fpd_wgrad_t& a, hipStream_t st);
int fpd_wgrad_tile_variant_of(const fpd_wgrad_t& a);      // the wgrad_tile_kernel instantiation that launch runs (packed, see wgrad_tile.hip), -1: declined or handed to wgrad3
int fpd_wgrad_tile_launches();                     // "wgrad_tile_launches"
int fpd_wgrad3_launches();                         // "wgrad3_launches" (wgrad3.hip: the launches fpd_wgrad_tile_launch handed over)
int fpd_wgrad_mfma_partials(const fpd_wgrad_t& a);
int fpd_wgrad_mfma_launch(const fpd_wgrad_t& a, hipStream_t st);
int fpd_wgrad_smallc_partials(const fpd_wgrad_t& a);
int fpd_wgrad_smallc_launch(const fpd_wgrad_t& a, hipStream_t st);
int fpd_wgrad_naive_partials(const fpd_wgrad_t& a);
int fpd_wgrad_naive_launch(const fpd_wgrad_t& a, hipStream_t st);
int fpd_wreduce_launch(const fpd_wreduce_entry_t* table, int n, int64_t max_elems, hipStream_t st);

// ---- stem ----
int fpd_stem_forward_s2d_launch(const fpd_stem_t& a, hipStream_t st);
bool fpd_stem_forward_s2d_takes_act(const fpd_stem_t& a);
int fpd_stem_s2d_option(int which, int value);      // which: 0 = "stem_act", 1 = "stem_blocks" (return the previous value), 2 = "stem_s2d_launches"
int fpd_stem_blocks(int dflt);                      // the grid / slab cap of a persistent stem launch whose own cap is dflt ("stem_blocks")
int fpd_stem_mfma_launches();                       // "stem_mfma_launches"
int fpd_stem_wgrad_s2d_partials(const fpd_stem_t& a);
int fpd_stem_wgrad_s2d_launch(const fpd_stem_t& a, hipStream_t st);
int fpd_stem_forward_mfma_launch(const fpd_stem_t& a, hipStream_t st);
int fpd_stem_wgrad_mfma_partials(const fpd_stem_t& a);
int fpd_stem_wgrad_mfma_launch(const fpd_stem_t& a, hipStream_t st);
int fpd_stem_forward_launch(const fpd_stem_t& a, hipStream_t st);
int fpd_stem_wgrad_partials(const fpd_stem_t& a);
int fpd_stem_wgrad_launch(const fpd_stem_t& a, hipStream_t st);

// ---- everything else: one kernel each ----
int fpd_bneck_fused_launch(const fpd_bneck_t& a, hipStream_t st);
int fpd_bneck_fused_pair_launch(const fpd_bneck_t& a, const fpd_bneck_t& b, hipStream_t st);
int fpd_bneck_fold_launch(const fpd_bneck_t& a, float* out, hipStream_t st);
// up-add formed on load (fpd_bneck_t.x2): nullptr = dimensions served, else the reason; the launch walks the same decision
const char* fpd_bneck_upadd_why_not(const fpd_bneck_t& a);
int fpd_bneck_upadd_option(int value);      // >= 0: set; returns the previous value
int fpd_bneck_blocks_option(int value);     // >= 1: set the grid cap (GridCap); returns the previous value
int fpd_head_blocks_option(int value);
int fpd_head_fused_launch(const fpd_head_t& a, hipStream_t st);
int fpd_head_fold_launch(const fpd_head_t& a, float* out, hipStream_t st);
int fpd_pck_launch(const fpd_pck_t& a, hipStream_t st);
int fpd_flip_w_launch(const float* x, float* y, int64_t rows, int W, hipStream_t st);
int fpd_flip_merge_launch(const fpd_flipmerge_t& p, hipStream_t st);
int fpd_final_preds_launch(const fpd_finalpreds_t& p, hipStream_t st);
int fpd_val_post_launch(const fpd_val_post_t& p, hipStream_t st);
int fpd_dark_launch(const fpd_dark_t& p, hipStream_t st);                         // csrc/dark.hip
int fpd_vis_minmax_launch(const fpd_vis_minmax_t& p, hipStream_t st);             // csrc/vis.hip
int fpd_vis_max_preds_launch(const fpd_vis_max_preds_t& p, hipStream_t st);
int fpd_vis_joints_grid_launch(const fpd_vis_joints_grid_t& p, hipStream_t st);
int fpd_vis_heatmap_grid_launch(const fpd_vis_heatmap_grid_t& p, hipStream_t st);
int64_t fpd_vis_joints_canvas_bytes(const fpd_vis_joints_grid_t& p);
int fpd_render_targets_launch(const fpd_targets_t& a, hipStream_t st);
int fpd_warp_affine_launch(const fpd_warp_t& a, hipStream_t st);
int fpd_render_targets_w_launch(const fpd_targets_w_t& a, hipStream_t st);
int fpd_render_targets_unbiased_launch(const fpd_targets_unbiased_t& a, hipStream_t st);
int fpd_warp_affine_aug_launch(const fpd_warp_aug_t& a, hipStream_t st);
int fpd_augment_params_launch(const fpd_augment_t& a, hipStream_t st);
int fpd_oks_nms_launch(const fpd_oks_nms_t& a, hipStream_t st);
int fpd_coco_match_launch(const fpd_coco_match_t& a, hipStream_t st);            // csrc/coco_eval.hip
int fpd_coco_accumulate_launch(const fpd_coco_accum_t& a, hipStream_t st);
int fpd_elementwise_launch(const fpd_ew_t& a, hipStream_t st);
int fpd_elementwise_pair_launch(const fpd_ew_t& a, const fpd_ew_t& b, hipStream_t st);
int fpd_affsum_launch(const fpd_affsum_t& a, hipStream_t st);
// merged BN-backward apply + pool backward (elementwise.hip): nullptr = served, else the reason; the launch walks the same decision
const char* fpd_ew_merge_why_not(const fpd_ew_merge_t& m);
int fpd_ew_merge_launch(const fpd_ew_merge_t& m, hipStream_t st);
int fpd_ew_merge_option(int value);      // >= 0: set; returns the previous value
int fpd_ew_merge_blocks_option(int value);      // >= 1: set the grid cap of the merged launches; returns the previous value
int fpd_ew_blocks_option(int value);      // >= 1: grid cap of fpd_elementwise_launch (each half of a pair launch) and fpd_affsum_launch, 0: none (default); returns the previous value
int fpd_loss_launch(const fpd_loss_t& a, hipStream_t st);
int fpd_loss_geometry_of(const fpd_loss_t& a, int* vectorised, int* blocks, int* tiles_per_block);      // the kernel and grid of that launch
int fpd_loss_ohkm_launch(const fpd_loss_ohkm_t& a, hipStream_t st);      // csrc/loss_ohkm.hip: two launches
int64_t fpd_loss_ohkm_scratch_size(const fpd_loss_t& a);
int fpd_loss_kl_launch(const fpd_loss_kl_t& a, hipStream_t st);          // csrc/loss_kl.hip: two launches
int64_t fpd_loss_kl_scratch_size(const fpd_loss_t& a);
int fpd_adam_launch(const fpd_adam_t& a, hipStream_t st);
int fpd_sgd_launch(const fpd_sgd_t& a, hipStream_t st);
int fpd_adamw_launch(const fpd_adamw_t& a, hipStream_t st);              // csrc/adamw.hip: the streaming kernel + the counter's tick
int fpd_adamw_geometry_of(const fpd_adamw_t& a, int* blocks, int64_t* nvec);  // its validation, grid and 16-byte vectors
int fpd_ema_launch(const fpd_ema_t& a, hipStream_t st);                  // csrc/ema.hip: the streaming kernel + the counter's tick
int fpd_ema_geometry_of(const fpd_ema_t& a, int* blocks, int64_t* nvec);      // its validation, grid and vectors per segment
int fpd_grad_clip_launch(const fpd_grad_clip_t& a, hipStream_t st);      // csrc/grad_clip.hip: sums of squares, finalise, in-place scale
int fpd_grad_clip_geometry_of(const fpd_grad_clip_t& a, int* blocks, int64_t* nvec);      // its validation, grid and 16-byte vectors
int64_t fpd_grad_clip_scratch_size(int64_t n);
int fpd_grad_accum_launch(const fpd_grad_accum_t& a, hipStream_t st);    // csrc/grad_accum.hip: one streaming launch, three modes
int fpd_grad_accum_geometry_of(const fpd_grad_accum_t& a, int* blocks, int64_t* nvec);    // its validation, grid and 16-byte vectors
int fpd_weight_prep_launch(const fpd_wprep_entry_t* table, int n, int64_t max_elems, int dtype, hipStream_t st);
int fpd_bn_update_running_launch(const fpd_bnupd_entry_t* table, int n, hipStream_t st);
int fpd_cast_launch(const void* src, void* dst, int64_t n, int sd, int dd, hipStream_t st);
int fpd_nchw_to_nhwc_launch(const float* src, void* dst, int N, int C, int H, int W, int dtype, hipStream_t st);
int fpd_nhwc_to_nchw_launch(const void* src, float* dst, int N, int C, int H, int W, int dtype, hipStream_t st);
