/*
 * fpd_amd.h -- C ABI of the MI355X (gfx950) Fast-Pose-Distillation training path.
 *
 * The reference (ilovepose/fast-human-pose-estimation.pytorch) has NO native/FFI interface on
 * this path: its boundary is the Python module API (lib/models/hourglass.py:170-197,
 * lib/core/loss.py:15-39, lib/core/function.py:99-187) and all arithmetic is torch.nn
 * (cuDNN/ATen).  This header therefore DEFINES the boundary a maintainer would bind from
 * Python (ctypes stub in INTEGRATION.md).  Each entry point names the reference call site
 * whose arithmetic it replaces.
 *
 * Conventions:
 *   - plain pointers + sizes, no torch types; the CALLER owns every buffer (incl. workspaces);
 *   - every call is asynchronous on the given hipStream_t, never synchronises, never allocates;
 *   - return 0 on success, negative on error; fpd_last_error() gives a thread-local message;
 *   - activations are NHWC ("channels last"), dtype FPD_F32 or FPD_BF16; conv weights are
 *     K,R,S,C (the reference's OIHW tensor stored channels-last); statistics are exact fixed-point sums (fpd_stat_t).
 */
#ifndef FPD_AMD_H
#define FPD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fpd_stream_t; /* hipStream_t */

enum { FPD_F32 = 0, FPD_BF16 = 1 };
/* Every per-channel statistics buffer (BN forward {sum, sumsq}; BN backward {sum dz, sum dz*xhat}) holds
 * FPD_STATS_REPLICAS independent partial copies.  Producer block b adds into replica b % R (thousands of blocks adding
 * into ONE address serialise at ~20 ns per atomic); consumers sum the replicas.
 * The sums are EXACT and therefore independent of the order in which the blocks' contributions arrive (a training step
 * is bit-repeatable): a block's fp64 partial v is added as two 64-bit INTEGER limbs
 *     hi = rint(v * 2^20)                     units of 2^-20  (|v| clamped to 2^42)
 *     lo = rint((v - hi * 2^-20) * 2^60)      units of 2^-60  (|lo| <= 2^39)
 * with integer atomics (associative, unlike floating-point ones; measured on MI355X: same cost as an fp64 atomic pair),
 * value = hi * 2^-20 + lo * 2^-60.  BOUND: a limb sum is a 64-bit integer, so one (replica, sum, channel) takes up to
 * 2^24 contributions whatever their signs (|lo| <= 2^39 each) and a total of magnitude < 2^42; both are checked nowhere
 * at run time -- the producers of this library add at most 2^17 contributions per channel (ABI version 2; version 1 used
 * hi units of 2^-8, which wrapped after 4 096 worst-case addends).  Layout of one buffer over C channels: fpd_stat_t [R][2 sums][2 limbs: hi, lo][C]
 * (FPD_STATS_WORDS(C) 64-bit words); the caller zeroes it (all-zero bytes = all-zero sums). */
#ifndef FPD_STATS_REPLICAS
#define FPD_STATS_REPLICAS 4
#endif
typedef int64_t fpd_stat_t;
#define FPD_STATS_WORDS(C) ((int64_t)FPD_STATS_REPLICAS * 4 * (C))
enum { FPD_BN_NONE = 0, FPD_BN_TRAIN = 1, FPD_BN_EVAL = 2 };
enum { FPD_EPI_PLAIN = 0, FPD_EPI_BNRELU_BWD = 1 };
enum { FPD_BACKEND_MFMA = 0, FPD_BACKEND_NAIVE = 1, FPD_BACKEND_MFMA_GENERIC = 2 };
/* MFMA: halo-tile kernel where it applies, else the generic MFMA kernel, else the direct kernel;
 * MFMA_GENERIC skips the halo-tile kernel; NAIVE forces the direct kernels (cross-check). */

/* nn.BatchNorm2d(momentum=0.1) (hourglass.py:18-25,118,162) applied on the fly while a consumer
 * loads the tensor: a = relu?(x*scale+shift).  TRAIN: scale/shift derive from the batch
 * statistics `stats` = {sum[C], sumsq[C]} accumulated by the tensor's producer; EVAL: from the
 * running estimates. */
typedef struct {
    int32_t mode;          /* FPD_BN_* */
    int32_t relu;          /* apply ReLU after the affine (hourglass.py:28) */
    float eps;
    int32_t _pad;
    const fpd_stat_t* stats; /* TRAIN: statistics buffer over C: sum, sum of squares over N*H*W (layout: fpd_stat_t above) */
    const float* gamma;    /* [C] */
    const float* beta;     /* [C] */
    const float* running_mean; /* EVAL: [C] */
    const float* running_var;  /* EVAL: [C] */
} fpd_bn_t;

/* nn.Conv2d forward as an implicit GEMM (hourglass.py:20,23,27,116,135-137,143-145,163), with
 * the preceding BN+ReLU fused on the input, and bias / residual add (hourglass.py:50,189) /
 * batch statistics of the result (for the next train-mode BN) fused on the output.
 * The same kernel computes the data gradient of a stride-1 conv when given the flipped,
 * IO-swapped weights; epi = FPD_EPI_BNRELU_BWD then masks the result with the forward ReLU of
 * tensor `epi_x` and accumulates the two BN-backward sums {sum dz, sum dz*xhat} into epi_stats. */
typedef struct {
    int32_t N, H, W, C;    /* input  [N,H,W,C] */
    int32_t K, R, S;       /* output channels, filter height/width */
    int32_t stride, pad;
    int32_t P, Q;          /* output [N,P,Q,K] */
    int32_t dtype;         /* FPD_F32 / FPD_BF16: x, w, residual, y, epi_x */
    int32_t epi;           /* FPD_EPI_* */
    int32_t _pad;
    const void* x;
    const void* w;         /* [K][R][S][C] */
    const float* bias;     /* [K] or NULL */
    const void* residual;  /* [N,P,Q,K] or NULL (may alias y) */
    void* y;
    fpd_stat_t* out_stats; /* statistics buffer over K += {sum y, sum y^2}, or NULL */
    fpd_bn_t bn;           /* prologue on x (mode NONE = raw x) */
    const void* epi_x;     /* BNRELU_BWD: forward tensor normalised by epi_bn, [N,P,Q,K] */
    fpd_bn_t epi_bn;       /* BNRELU_BWD: its (train-mode) BN */
    fpd_stat_t* epi_stats; /* BNRELU_BWD: statistics buffer over K += {sum dz, sum dz*xhat} */
    /* FUSED WEIGHT GRADIENT (optional; BNRELU_BWD data gradient of a 1x1 convolution only): this launch is the data gradient
     * of a forward convolution y = W * a(u), a(u) = relu?(bn(u)); it reads x = dy and epi_x = u anyway, so it can form the
     * forward convolution's weight gradient dW[k][c] = sum_pixels dy[.,k] * a(u)[.,c] (k < C of this launch, c < K of this
     * launch) and bias gradient sum_pixels dy[.,k] on the way, saving the separate fpd_conv_wgrad() launch and its HBM reads.
     * Persistent block range b stores its partial sums to wg_partial + b*wg_stride (layout [C][K] floats, then [C] bias
     * sums when wg_bias); fpd_wgrad_reduce() adds the slabs in order.  The number of slabs is fpd_conv_fused_wgrad_partials()
     * (0 = this shape / configuration is not served: leave wg_partial NULL and call fpd_conv_wgrad()). */
    float* wg_partial;
    int64_t wg_stride;     /* floats between slabs, >= C*K + C */
    int32_t wg_bias;       /* also accumulate the bias gradient */
    int32_t wg_count;      /* slabs the caller provided behind wg_partial = what fpd_conv_fused_wgrad_partials() returned when the
                            * workspace was sized; the launch fails (instead of writing past it) if its geometry has changed since
                            * -- e.g. fpd_set_option("conv_pp_blocks") between the query and the launch */
    /* FOLDED BN-BACKWARD APPLY (optional; BNRELU_BWD data gradients served by the persistent kernel only, bn.mode NONE): x is
     * not the operand itself but the masked gradient g that reached a train-mode BatchNorm whose input was fold_x = u, with
     * the two sums {sum g, sum g*xhat} in fold_stats.  The launch evaluates the BN backward on the way into its operand image,
     *     dy = gamma*invstd * (g - mean(g) - xhat*mean(g*xhat)),   xhat = (u - mean(u)) * invstd,
     * rounds it once (like the stand-alone FPD_EW_BN_BWD_APPLY it replaces: one launch and three tensor passes fewer) and
     * convolves THAT; if fold_out is given the evaluated operand is also written out once ([N,H,W,C], for a separate
     * weight-gradient launch), fold_dgamma / fold_dbeta receive sum g*xhat / sum g.  fpd_conv_fold_supported() tells
     * whether a launch is served (0: leave fold_x NULL and issue the apply). */
    const void* fold_x;
    fpd_bn_t fold_bn;
    const fpd_stat_t* fold_stats;
    void* fold_out;
    float* fold_dgamma;
    float* fold_dbeta;
    /* SECOND 1x1 SOURCE (optional; forward FPD_EPI_PLAIN launches of the streaming 1x1 kernel only): the downsample branch of a
     * Bottleneck (hourglass.py:45-50) formed in the launch of conv3 instead of a launch of its own.  Exactly the two launches
     * it replaces, rounding points included:
     *     skip = round(W2 * x2 + bias2)              (the plain launch: x2 raw, no prologue)
     *     y    = round((W * a(x) + skip) + bias)     (the launch with residual = skip)
     * residual must be NULL.  Domain: BF16, C2 == C in {32, 64}, K == 2C, every pointer 16-byte aligned, no pair launch.
     * fpd_conv_skip_supported() tells whether a launch is served (0: leave x2 NULL and issue the two launches). */
    const void* x2;        /* [N,H,W,C2] */
    const void* w2;        /* [K][1][1][C2] */
    const float* bias2;    /* [K] or NULL */
    int32_t C2;
    int32_t _pad2;
} fpd_conv_t;

/* A whole pre-activation Bottleneck of a FROZEN network in one launch (hourglass.py:32-52 with eval-mode BN, no
 * downsample branch):  y = x + conv3(relu(bn3(conv2(relu(bn2(conv1(relu(bn1(x)))))))))  with conv1 1x1 C->P,
 * conv2 3x3 P->P pad 1, conv3 1x1 P->C.  Both P-channel intermediates stay in LDS (rounded to bf16 once, after
 * bias+BN+ReLU).  Domain: dtype BF16, C == 2P, P in {64,128}, W a power of two in [4,64], H*W a multiple or a divisor
 * of 128, every BN in EVAL mode; fpd_bottleneck_forward() returns an error outside it (callers then issue the three
 * fpd_conv_forward() calls).
 * UP-ADD ON LOAD (optional, x2 != NULL): the Bottleneck that follows an hourglass level's `up1 + up(low)` (hourglass.py:80-92)
 * forms that sum where it reads its input instead of reading a tensor a FPD_EW_UPADD_FWD launch materialised:
 *     x'[n,i,j,:] = round(x[n,i,j,:] + x2[n,i/2,j/2,:]),   y = x' + conv3(...(bn1(x')))
 * exactly the two launches it replaces, the rounding of the sum included.  Domain: the one above with W in {8,16,32,64} and H
 * even; y aliases neither source; no pair launch.  fpd_bneck_upadd_supported() tells whether such a launch is served (0: leave
 * x2 NULL and issue the two launches). */
typedef struct {
    int32_t N, H, W, C, P, dtype;
    int32_t _pad[2];
    const void* x;         /* [N,H,W,C] */
    void* y;               /* [N,H,W,C] (must not alias x: neighbouring tiles re-read x rows) */
    const void* w1;        /* [P][1][1][C] working-precision weights */
    const float* b1;       /* [P] or NULL */
    const void* w2;        /* [P][3][3][P] */
    const float* b2;
    const void* w3;        /* [C][1][1][P] */
    const float* b3;       /* [C] or NULL */
    fpd_bn_t bn1, bn2, bn3;
    /* optional [3C + 4P] floats written by fpd_bottleneck_fold(): the three BNs folded to scale/shift with the conv1/conv2
     * biases folded into the following shift, + b3.  A frozen model folds once; NULL = every block folds for itself. */
    const float* folded;
    const void* x2;        /* [N,H/2,W/2,C] low branch added to x on load, or NULL */
} fpd_bneck_t;

/* The inter-stack head of a FROZEN hourglass stack in one launch (hourglass.py:134-137,184-190 with eval-mode BN):
 *   a = relu(bn(fc(y0)));  score = score_conv(a);  next = x + fc_(a) + score_(score)        (all 1x1 convolutions)
 * `a` stays in LDS (rounded to bf16 once); score is rounded to bf16 once (it is an output) and reused from LDS.
 * next == NULL (last stack): only score is produced and w_fc2 / w_score2 / x may be NULL.
 * Domain: dtype BF16, C == 256, J == 16; fpd_head_forward() returns an error outside it. */
typedef struct {
    int32_t N, H, W, C, J, dtype;
    int32_t _pad[2];
    const void* y0;        /* [N,H,W,C] output of the stack's last Bottleneck */
    const void* x;         /* [N,H,W,C] the stack's input (residual), or NULL */
    void* score;           /* [N,H,W,J] */
    void* next;            /* [N,H,W,C] input of the next stack, or NULL */
    const void* w_fc;      /* [C][1][1][C] */
    const float* b_fc;
    const void* w_score;   /* [J][1][1][C] */
    const float* b_score;
    const void* w_fc2;     /* fc_: [C][1][1][C] */
    const float* b_fc2;
    const void* w_score2;  /* score_: [C][1][1][J] */
    const float* b_score2;
    fpd_bn_t bn;           /* fc.1, EVAL */
    const float* folded;   /* optional [3C+32] floats written by fpd_head_fold() */
} fpd_head_t;
int fpd_head_forward(const fpd_head_t* a, fpd_stream_t stream);
int fpd_head_fold(const fpd_head_t* a, fpd_stream_t stream);

/* Two INDEPENDENT convolutions issued as one launch (the parallel up-/low-branch bottlenecks of an hourglass level,
 * hourglass.py:80-88, have identical channel shapes at full and half resolution): fpd_conv_forward_pair() runs them in a
 * single kernel when both are in the halo-tile domain with equal dtype/C/K/R, else one after the other. */
typedef struct { fpd_conv_t a, b; } fpd_conv_pair_t;

/* Two independent frozen Bottlenecks as one launch (same P; else / outside the domain: an error, see fpd_bneck_t). */
typedef struct { fpd_bneck_t a, b; } fpd_bneck_pair_t;

/* Weight + bias gradient of the same conv (autograd of hourglass.py convs): dw[K][R][S][C] +=
 * sum_pixels dy * a(x), dbias[K] += sum_pixels dy; the caller zeroes dw/dbias.  DETERMINISTIC: no floating-point
 * atomics -- every sum is formed in a fixed order, so two runs on the same inputs give identical bytes. */
typedef struct {
    int32_t N, H, W, C, K, R, S, stride, pad, P, Q, dtype;
    const void* x;         /* forward input (pre-BN) */
    const void* dy;        /* [N,P,Q,K] */
    float* dw;             /* [K][R][S][C] fp32 */
    float* dbias;          /* [K] or NULL */
    fpd_bn_t bn;           /* forward prologue, recomputed */
    /* two-stage reduction (what a training plan uses): block / pixel chunk b stores its accumulator to
     * partial + b*partial_stride (layout of dw, bias partials behind it); fpd_wgrad_reduce() adds the slabs to dw in slab
     * order afterwards.  The number of slabs written for these dimensions is fpd_wgrad_num_partials() (>= 1 for every
     * supported shape).  partial == NULL: the launch uses ONE block per output element group, which adds into dw
     * directly -- same result, no workspace, but no parallelism over the pixel axis (small problems / tests). */
    float* partial;
    int64_t partial_stride; /* floats between slabs, >= K*R*S*C + K (bias partials sit behind the weights) */
} fpd_wgrad_t;

/* Stem: Conv2d(3, K, 7, stride 2, pad 3) (hourglass.py:116,172) reading the fp32 NCHW image. */
typedef struct {
    int32_t N, H, W, K, P, Q, dtype, _pad;
    const float* x;        /* [N,3,H,W] fp32 NCHW */
    const float* w;        /* [K][7][7][3] fp32 */
    const float* bias;     /* [K] */
    void* y;               /* [N,P,Q,K] */
    fpd_stat_t* out_stats; /* statistics buffer over K, or NULL */
    const void* dy;        /* wgrad: [N,P,Q,K] */
    float* dw;             /* wgrad: [K][7][7][3] */
    float* dbias;          /* wgrad: [K] */
    float* partial;        /* wgrad: slabs of the two-stage reduction (see fpd_wgrad_t), fpd_stem_wgrad_num_partials() of them, or NULL */
    int64_t partial_stride; /* floats between slabs, >= K*147 + K */
    /* forward, optional (mode FPD_BN_EVAL; FPD_BN_NONE = off): the frozen network's bn1 + ReLU (hourglass.py:173-174) applied in
     * the epilogue, y = round(relu?(scale * float(round(acc + bias)) + shift)) -- the inner rounding is kept, so y holds the
     * bits of fpd_stem_forward() followed by FPD_EW_BNRELU_FWD.  out_stats must be NULL.  fpd_stem_act_supported() tells whether
     * the launch is served (0: leave the mode NONE and issue the elementwise op). */
    fpd_bn_t act;
} fpd_stem_t;

/* Elementwise / pooling ops on NHWC tensors.  `op` selects the function:
 *  BNRELU_FWD   y = relu(bn(x)); out_stats += stats(y)                  (hourglass.py:173-174)
 *  BNRELU_BWD_R dz = dy * (yfwd > 0) -> y ; bstats += {sum dz, sum dz*xhat(x)}   (yfwd = relu(bn(x)), or x2 when given: the
 *               forward output of an HRNet block tail relu(bn(conv) + skip), pose_hrnet.py:52-57 -- mask and sums in one pass)
 *  BN_BWD_APPLY y = add + gamma*invstd*(dz - s1/n - xhat(x)*s2/n)       (BatchNorm backward; dz in `dy`)
 *  MAXPOOL_FWD  y = maxpool2x2(x); out_stats += stats(y)               (hourglass.py:82,177)
 *  MAXPOOL_BWD  y = add + (x is the first max of its window ? dy : 0)
 *  UPADD_FWD    y = x + nearest_up2(x2); out_stats += stats(y)         (hourglass.py:90-91)
 *  SUMPOOL      y = add + sum2x2(x)                                    (Upsample backward)
 *  ADD          y = x + x2
 *  RELU_MASK    y = dy * (x > 0)   (x = the forward OUTPUT of a ReLU; pose_hrnet.py:55,96,261 autograd)
 *  DILATE2      y[n,2p,2q,:] = x[n,p,q,:], zero elsewhere; N,H,W = shape of y (even H,W).  The data gradient of a
 *               stride-2 convolution (pose_hrnet.py:223-242,349-372) is the stride-1 convolution of this tensor.
 * BNRELU_BWD_R with y == NULL accumulates the two sums only.
 */
enum {
    FPD_EW_BNRELU_FWD = 0, FPD_EW_BNRELU_BWD_R = 1, FPD_EW_BN_BWD_APPLY = 2, FPD_EW_MAXPOOL_FWD = 3,
    FPD_EW_MAXPOOL_BWD = 4, FPD_EW_UPADD_FWD = 5, FPD_EW_SUMPOOL = 6, FPD_EW_ADD = 7, FPD_EW_RELU_MASK = 8,
    FPD_EW_DILATE2 = 9
};
typedef struct {
    int32_t op, dtype;
    int32_t N, H, W, C;    /* shape of the LARGER spatial tensor involved (pool input / up output) */
    const void* x;         /* see table (BNRELU_FWD, UPADD_FWD, ADD: may alias y -- a thread reads the element it then writes) */
    const void* x2;
    const void* dy;
    const void* add;       /* optional accumulate source (may alias y) */
    void* y;
    fpd_stat_t* out_stats; /* statistics buffer over C, or NULL */
    fpd_stat_t* bstats;    /* BN-backward sums: statistics buffer over C */
    float* dgamma;         /* BN_BWD_APPLY: optional [C] <- sum dz*xhat (grad of BN weight) */
    float* dbeta;          /* BN_BWD_APPLY: optional [C] <- sum dz      (grad of BN bias) */
    fpd_bn_t bn;
} fpd_ew_t;

/* MERGED BN-BACKWARD APPLY + 2x2 POOL BACKWARD: a FPD_EW_BN_BWD_APPLY that carries a residual `add`, evaluated inside the
 * pool-backward op that reads its result first -- one launch where the plan had two, and the tensor between them is not
 * re-read (kind 0: not even written).  The members are the descriptors of the launches replaced, as they would have been
 * issued; the result holds their bits: an apply is rounded to the storage type exactly where its own launch rounded it, and
 * the rounded value enters the pool op's arithmetic unchanged.
 *  FPD_EWM_MAXPOOL_BWD  the apply pair in front of a max-pool backward (the up / low branch of an hourglass level):
 *      a_i = round(apply_full(full.dy[i], full.x[i]) + full.add[i])     the four pixels of a window   (has_full)
 *      b   = round(apply_half(half.dy, half.x) + half.add)              the pooled pixel
 *      pool.y[i] = round((i is the first maximum of pool.x's window in scan order ? b : 0) + a_i)
 *    has_full: pool.add == full.y, pool.x == full.x, same dims; a_i is not stored.  !has_full: `full` is ignored and a_i =
 *    pool.add[i] (or 0).  Always pool.dy == half.y, half dims = (N, H/2, W/2, C); b is not stored.
 *  FPD_EWM_SUMPOOL      an apply in front of the nearest-up-sampling backward (`half` and has_full are ignored):
 *      dx_i = round(apply_full(full.dy[i], full.x[i]) + full.add[i])  -> full.y (stored: later ops read it)
 *      pool.y = round(pool.add + ((dx_0 + dx_1) + (dx_2 + dx_3)))     pool.x == full.y, same dims
 * dgamma / dbeta of every apply present are written as its own launch writes them.  No output may be one of the inputs
 * (pointer equality; the members' "may alias y" does not carry over).  fpd_ew_merge_supported() tells whether a launch is
 * served (0: issue the member launches). */
enum { FPD_EWM_MAXPOOL_BWD = 0, FPD_EWM_SUMPOOL = 1 };
typedef struct {
    int32_t kind;          /* FPD_EWM_* */
    int32_t has_full;      /* MAXPOOL_BWD: the full-resolution apply is present */
    fpd_ew_t full;         /* FPD_EW_BN_BWD_APPLY on [N,H,W,C], the pool op's dims */
    fpd_ew_t half;         /* MAXPOOL_BWD: FPD_EW_BN_BWD_APPLY on [N,H/2,W/2,C] */
    fpd_ew_t pool;         /* FPD_EW_MAXPOOL_BWD / FPD_EW_SUMPOOL */
} fpd_ew_merge_t;
int fpd_ew_merge(const fpd_ew_merge_t* a, fpd_stream_t stream);
/* 1 if fpd_ew_merge() would serve this launch (pure host code: the members' ops, dims, dtype, wiring and aliasing are looked
 * at, nothing is dereferenced); 0 otherwise.  Process-wide switch: FPD_EW_MERGE=0 / fpd_set_option("ew_merge", 0). */
int fpd_ew_merge_supported(const fpd_ew_merge_t* a);

/* y = relu?( sum_j a_j(up_j(x_j)) ): the tail of an HRNet block (pose_hrnet.py:52-57,93-98: relu(bn(conv) + skip)), a fuse
 * layer (:252-265: relu(sum of identity / 1x1-conv+BN+nearest-up / strided-conv+BN terms)) or a transition output (:349-372)
 * in ONE pass.  Term j is x_j[n, h/up_j, w/up_j, :] (nearest up-sampling by up_j in {1,2,4,8}), normalised by bn_j (mode
 * NONE = identity; TRAIN statistics cover the N*(H/up)*(W/up) pixels of x_j; bn_j.relu applies to the term).  The sum is
 * rounded to the storage type once. */
#define FPD_AFFSUM_MAX 4
typedef struct { const void* x; fpd_bn_t bn; int32_t up; int32_t _pad; } fpd_affterm_t;
typedef struct {
    int32_t N, H, W, C;    /* output shape [N,H,W,C] */
    int32_t dtype, relu, nterms, _pad;
    fpd_affterm_t t[FPD_AFFSUM_MAX];
    void* y;
} fpd_affsum_t;
int fpd_affsum(const fpd_affsum_t* a, fpd_stream_t stream);

/* [N,C,H,W] fp32 image -> [N,H,W,C] activation as a plan op (HRNet stem: its first convolution is a generic NHWC conv) */
typedef struct { const float* src; void* dst; int32_t N, C, H, W, dtype, _pad; } fpd_layout_t;

/* JointsMSELoss pose + KD over all stacks, forward and backward in one pass
 * (lib/core/loss.py:21-39 called 2*S times at lib/core/function.py:128-134):
 *   pose = sum_s 0.5/(B*J*hw) sum w^2 (p_s-g)^2 ; kd likewise against the teacher map t;
 *   dout_s = w^2 [(1-alpha)(p_s-g) + alpha (p_s-t)] / (B*J*hw).
 * use_target_weight=False (loss.py:30-37) = a weight buffer of ones. */
#define FPD_MAX_STACKS 8
typedef struct {
    int32_t B, J, H, W, S, dtype;
    int32_t target_nchw;   /* 1: target is [B,J,H,W] (reference loader layout); 0: [B,H,W,J] */
    float alpha;
    const void* out[FPD_MAX_STACKS];  /* student maps, NHWC [B,H,W,J] */
    void* dout[FPD_MAX_STACKS];       /* gradients, same layout (NULL = forward only) */
    const void* teacher;   /* NHWC [B,H,W,J] in dtype */
    const float* target;   /* fp32 */
    const float* weight;   /* [B,J] fp32 */
    double* losses;        /* [2] += {pose, kd}; caller zeroes */
    float grad_scale;      /* extra factor on dout (1/world for DP averaging), normally 1 */
    int32_t _pad;
    const float* weight_kd; /* optional [B,J]: weights of the distillation term when its criterion's use_target_weight
                             * differs from the pose criterion's (tools/fpd_train.py:145-147,177-179); NULL = `weight` */
} fpd_loss_t;

/* JointsOHKMMSELoss (online hard keypoint mining, lib/core/loss.py:42-84) for either term of fpd_loss_t, all stacks, forward and
 * backward in two launches.  Per criterion call (stack s, term, maps p against r = target / teacher map, weights w):
 *   L[n,j] = 0.5 w[n,j]^2 / hw * sum_x (p - r)^2 ;  sel(n) = the k joints with the largest L[n,:] ;  loss = 1/(B k) sum_n sum_{j in sel(n)} L[n,j]
 *   dout_s = grad_scale [(1-alpha) m_pose w^2 (p_s-g) / (B k_pose hw) + alpha m_kd w_kd^2 (p_s-t) / (B k_kd hw)],  m = [j in sel(n)].
 * torch.topk leaves the order of equal values open; here the LOWER joint index wins among equal L.  k = J keeps every joint:
 * that term is JointsMSELoss (a mixed pair of criteria = one k below J, the other J).  base.losses keeps {pose, kd} (caller
 * zeroes); no other buffer needs zeroing, every sum is formed in a fixed order (bit-repeatable).  J <= 32. */
typedef struct {
    fpd_loss_t base;
    int32_t topk_pose, topk_kd;   /* in [1, J]; J = every joint = JointsMSELoss */
    void* scratch;         /* fpd_loss_ohkm_scratch_bytes(&base) bytes, 8-byte aligned: partial row sums, double [B][chunks][S][2][J] */
    int64_t scratch_bytes;
    uint32_t* masks;       /* optional [S][2][B]: bit j = joint j of that (stack, term, sample) was kept */
} fpd_loss_ohkm_t;

/* JointsKLDLoss (soft-label KL over the spatial softmax of a heat map) for either term of fpd_loss_t, the other staying
 * JointsMSELoss; all stacks, forward and backward in two launches.  Per criterion call (stack map s against r = target / teacher
 * map, weight w, temperature T > 0), with p = softmax(s/T), q = softmax(r/T) over the hw pixels of that one map:
 *   L[n,j] = w[n,j] T^2 sum_x q_x ((r_x - s_x)/T - lse(r/T) + lse(s/T)) ;  loss = 1/(B J) sum_{n,j} L[n,j] ;
 *   d loss / d s_x = w[n,j] T (p_x - q_x) / (B J).
 * The weight enters ONCE (not squared as in the MSE terms).  Both softmaxes subtract the row maximum; q_x == 0 contributes an
 * exact 0 and no logarithm of a probability is taken.  dout_s = grad_scale [(1-alpha) dpose_s + alpha dkd_s] with each term MSE
 * (fpd_loss_t's) or KL.  base.losses keeps {pose, kd} (caller zeroes); no other buffer needs zeroing, every sum is formed in a
 * fixed order (bit-repeatable).  J <= 32.  Refused: both flags 0 (that is fpd_loss), a temperature <= 0 of a KL term. */
typedef struct {
    fpd_loss_t base;
    int32_t kl_pose, kl_kd;       /* 1: that term is KL, 0: MSE */
    float temp_pose, temp_kd;     /* temperature of a KL term (ignored for an MSE term) */
    void* scratch;         /* fpd_loss_kl_scratch_bytes(&base) bytes, 8-byte aligned: per-block row statistics */
    int64_t scratch_bytes;
} fpd_loss_kl_t;

/* torch.optim.Adam(lr) step over one flat fp32 arena (lib/utils/utils.py:69-73), optionally
 * emitting the bf16 working copy of the parameters. */
typedef struct {
    int64_t n;
    float* param; const float* grad; float* m; float* v;
    void* param_lp;        /* optional bf16 copy [n] */
    float lr, beta1, beta2, eps;
    float bias_corr1, bias_corr2;   /* 1-beta^t */
    float grad_scale;      /* multiply grads first (1/world_size) */
    int32_t _pad;
    const float* lr_dev;   /* optional: read lr from device memory (graph-replay safe) */
    int64_t* step_dev;     /* optional: device step counter t (bias corrections use t+1; incremented after) */
} fpd_adam_t;

/* torch.optim.AdamW(lr, betas, eps, weight_decay, amsgrad) step over one flat fp32 arena: fpd_adam_t's fields plus the
 * decoupled weight decay, the AMSGrad maximum and a bit mask of elements the decay skips.  Arithmetic in csrc/adamw_math.h,
 * one float32 rounding per operation, never fused:
 *   g = grad * grad_scale
 *   if element i decays:  p = p * keep,  keep = 1 - lr * weight_decay     (one multiply, one subtract; torch's
 *                                                                          param.mul_(1 - lr * wd), BEFORE the moments)
 *   m = beta1 * m + (1 - beta1) * g
 *   v = beta2 * v + ((1 - beta2) * g) * g
 *   vmax != NULL (AMSGrad):  vmax = (v > vmax || v != v) ? v : vmax;  vhat = vmax     (torch.maximum: a NaN wins)
 *   else                     vhat = v
 *   denom = sqrtf(vhat) * inv_sqrt_bc2 + eps
 *   p = p - step_size * (m / denom)
 * with bc1 = (float)(1 - pow((double)beta1, t)), bc2 likewise, t = *step_dev + 1 (pow in double on the float32 betas),
 * step_size = lr / bc1 and inv_sqrt_bc2 = 1 / sqrtf(bc2) in float32 -- fpd_adam's formula with two insertions.  The schedule
 * comes from lr_dev / step_dev, or, with a NULL pointer, from lr resp. bias_corr1 / bias_corr2 of the struct.  The decay is
 * decoupled only (no L2 term in the gradient); weight_decay = 0 with vmax is torch.optim.Adam(amsgrad = True).
 * Element i decays when weight_decay != 0 and bit (i & 31) of no_decay_bits[i >> 5] is clear; a NULL mask = the decay
 * covers the arena.  The mask has ceil(n / 32) words.  An element whose gradient, m and v are zero keeps m and v, and keeps a
 * parameter of +-0 (eps > 0): the alignment gaps of an arena need no mask bit.
 * One streaming launch (256 threads a block, the grid cap of the flat optimizer launches): 16-byte vectors where param, grad,
 * m, v and vmax are 16-byte aligned and param_lp 8-byte aligned, element by element otherwise, a scalar tail; a one-thread
 * launch behind it adds 1 to *step_dev, so no block reads a counter that has moved.
 * Refused before any launch: n < 0 or n >= 2^60, a null param / grad / m / v, weight_decay negative or not finite, a beta
 * outside [0, 1), eps negative or NaN, a misaligned pointer, any written range (param, m, v, vmax, param_lp, the counter)
 * overlapping any other range. */
typedef struct {
    int64_t n;
    float* param; const float* grad; float* m; float* v;
    void* param_lp;        /* optional bf16 copy [n], round to nearest even */
    float lr, beta1, beta2, eps;
    float bias_corr1, bias_corr2;   /* 1-beta^t, used when step_dev is NULL */
    float grad_scale;      /* multiply grads first (1/world_size) */
    int32_t _pad;
    const float* lr_dev;   /* optional: read lr from device memory (graph-replay safe) */
    int64_t* step_dev;     /* optional: device step counter t (bias corrections use t+1; incremented after) */
    float weight_decay;    /* >= 0, decoupled */
    int32_t _pad2;
    float* vmax;           /* optional [n]: non-NULL = AMSGrad, the running maximum of v */
    const uint32_t* no_decay_bits;   /* optional [ceil(n / 32)]: a set bit exempts that element from the decay */
} fpd_adamw_t;

/* torch.optim.SGD(lr, momentum, dampening = 0, weight_decay, nesterov, maximize = False) step over one flat fp32 arena
 * (lib/utils/utils.py:61-67), one launch:
 *   g = grad * grad_scale [+ weight_decay * param];  momentum != 0: buf = momentum * buf + g, g = nesterov ? g + momentum * buf : buf;
 *   param -= lr * g.
 * `buf` starts at zero (= torch's "first step copies the gradient" under dampening 0); momentum == 0 touches no buffer and
 * buf may be NULL.  The decay covers the whole arena (BN gamma / beta included: the reference passes one parameter group). */
typedef struct {
    int64_t n;
    float* param; const float* grad; float* buf;
    void* param_lp;        /* optional bf16 copy [n], round to nearest even */
    float lr, momentum, weight_decay;
    float grad_scale;      /* multiply grads first (1/world_size) */
    int32_t nesterov;
    int32_t _pad;
    const float* lr_dev;   /* optional: read lr from device memory (graph-replay safe) */
    int64_t* step_dev;     /* optional: device step counter, incremented once per step */
} fpd_sgd_t;

/* Exponential moving average of a model's state (timm ModelEmaV3 / the ExpMomentumEMA hook), one launch over up to
 * FPD_EMA_MAX_SEG flat fp32 segments (in practice the parameter arena and the BN running-statistics arena), arithmetic in
 * csrc/ema_math.h:
 *   u = *updates_dev + 1;  d = warmup ? min(decay, (1 + u) / (10 + u)) : decay  (float64);  w = (float)(1 - d)
 *   dst[i] = dst[i] + w * (src[i] - dst[i])          three float32 roundings, never fused
 *   copy_dst[i] = copy_src[i]                         (num_batches_tracked: integers are copied, not averaged)
 * A one-thread launch behind the kernel adds 1 to *updates_dev, so no block reads a counter that has moved.  A segment whose
 * src and dst are both 16-byte aligned moves 16-byte vectors (and up to 3 elements one by one), any other segment goes
 * element by element.  Refused before any launch: nseg outside 1..FPD_EMA_MAX_SEG, a negative n or copy_n, a null pointer
 * with a positive count, a null updates_dev, decay outside [0, 1), any written range (a dst, copy_dst, the counter)
 * overlapping any read or other written range (src == dst included). */
#define FPD_EMA_MAX_SEG 4
typedef struct { const float* src; float* dst; int64_t n; } fpd_ema_seg_t;
typedef struct {
    fpd_ema_seg_t seg[FPD_EMA_MAX_SEG];
    int32_t nseg, warmup;
    double decay;
    const int64_t* copy_src; int64_t* copy_dst; int64_t copy_n;   /* plain copy, may be NULL / 0 */
    int64_t* updates_dev;  /* updates done so far; read by every thread, incremented behind the kernel */
} fpd_ema_t;

/* torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type = 2, error_if_nonfinite = False) over one flat fp32 gradient
 * arena, scaled in place, so that every optimizer launch behind it works unchanged.  Arithmetic in csrc/grad_clip_math.h:
 *   S = sum (double)g[i] * (double)g[i];  norm = (float)sqrt(S);  coef = max_norm / (norm + 1e-6f);  coef > 1 -> 1 (NaN stays)
 *   g[i] = g[i] * coef                          skipped for the whole arena only when coef == 1 exactly
 * Three launches on the stream: per-block float64 sums of squares into partial[block] (256 threads a block, the grid cap of
 * the flat optimizer launches, 16-byte loads where `grad` is 16-byte aligned, element by element otherwise); one block that
 * adds the partials in index order and writes out[0] = norm, out[1] = coef, counters[0] += 1, counters[1] += (coef < 1),
 * counters[2] += !isfinite(norm); the scale.  No atomics: the result is a function of the values, n and the alignment.
 * max_norm = +inf measures without clipping.  n == 0 is legal: norm 0, coef 1.
 * Refused before any launch: n < 0 or n >= 2^60, a null grad with n > 0, a null out or partial, partial_bytes below
 * fpd_grad_clip_scratch_bytes(n), a misaligned pointer, max_norm NaN or <= 0, out / partial / counters overlapping grad or
 * each other. */
typedef struct {
    int64_t n; float* grad;          /* flat fp32 arena, scaled in place */
    float max_norm; int32_t _pad;    /* > 0, +inf allowed */
    double* partial; int64_t partial_bytes;   /* caller-owned, >= fpd_grad_clip_scratch_bytes(n), 8-byte aligned */
    float* out;                      /* [2]: norm, coef */
    int64_t* counters;               /* optional [3]: calls, clipped, non-finite */
} fpd_grad_clip_t;

/* Gradient accumulation over a window of micro-batches: one launch over two flat fp32 arenas of n elements, in one of three
 * modes (a field, so that a recorded plan op is fixed).  Arithmetic in csrc/grad_accum_math.h:
 *   FPD_ACCUM_FIRST  acc[i] = grad[i]              a copy of the bits; acc is not read, so it needs no zero-fill
 *   FPD_ACCUM_ADD    acc[i] = acc[i] + grad[i]     one float32 addition; grad is not written
 *   FPD_ACCUM_FIN    grad[i] = acc[i] * s          one float32 multiplication, s = *scale_dev; acc is not written
 * 256 threads a block, the grid cap of the flat optimizer launches, 16-byte vectors where both bases are 16-byte aligned and
 * element by element otherwise, a scalar tail, no atomics.  n == 0 is legal.
 * Refused before any launch: n < 0 or n >= 2^60, a null grad or acc with n > 0, a pointer that is not 4-byte aligned, grad
 * overlapping acc, scale_dev overlapping either arena, an unknown mode, a null scale_dev in FIN. */
enum { FPD_ACCUM_FIRST = 0, FPD_ACCUM_ADD = 1, FPD_ACCUM_FIN = 2 };
typedef struct {
    int64_t n;
    float* grad;                     /* read in FIRST and ADD, written in FIN */
    float* acc;                      /* written in FIRST, read and written in ADD, read in FIN */
    const float* scale_dev;          /* device float, read by FIN when the launch runs; may be null in FIRST and ADD */
    int32_t mode; int32_t _pad;
} fpd_grad_accum_t;

/* Per-conv working copies of the weights: cast to `dtype` in K,R,S,C order (forward operand)
 * and the flipped, IO-swapped C,R,S,K copy (data-gradient operand).  One launch for a table. */
typedef struct {
    const float* w;        /* master [K][R][S][C] fp32 */
    void* w_fwd;           /* [K][R][S][C] dtype, or NULL */
    void* w_bwd;           /* [C][R][S][K] dtype with r,s flipped, or NULL */
    int32_t K, R, S, C;
} fpd_wprep_entry_t;

/* Running-statistics update of train-mode BNs after a forward (torch: momentum 0.1, unbiased
 * variance; hourglass.py:10).  One launch for a table. */
typedef struct {
    const fpd_stat_t* stats; /* statistics buffer over C */
    float* running_mean; float* running_var; int64_t* num_batches_tracked;
    double count; float momentum; int32_t C;
} fpd_bnupd_entry_t;

/* dw[i] += sum_{b < count} partial[b*stride + i], i < n : second stage of the weight-gradient reduction, one
 * launch for a table of convolutions. */
typedef struct {
    const float* partial; float* dw; int64_t n; int64_t stride; int32_t count; int32_t _pad;
} fpd_wreduce_entry_t;

/* ---- single-op entry points (asynchronous on `stream`) ---- */
int fpd_conv_forward(const fpd_conv_t* a, fpd_stream_t stream);
int fpd_conv_forward_pair(const fpd_conv_pair_t* p, fpd_stream_t stream);
/* fused frozen Bottleneck (three convs + three eval-mode BN+ReLU + residual), see fpd_bneck_t */
int fpd_bottleneck_forward(const fpd_bneck_t* a, fpd_stream_t stream);
/* writes a->folded (must be non-NULL) from a's BN / bias pointers; rerun whenever those parameters change */
int fpd_bottleneck_fold(const fpd_bneck_t* a, fpd_stream_t stream);
int fpd_bottleneck_forward_pair(const fpd_bneck_pair_t* p, fpd_stream_t stream);
/* 1 if fpd_bottleneck_forward() serves a launch of these dimensions with a low-branch source (fpd_bneck_t.x2), else 0.  Pure host
 * code; reads N, H, W, C, P, dtype and the option "bneck_upadd" only, so it can be asked before the tensors have addresses. */
int fpd_bneck_upadd_supported(const fpd_bneck_t* a);
/* slabs the fused weight gradient of data-gradient launch `a` writes (see fpd_conv_t.wg_partial); 0 = not available.  For the
 * two convolutions of a pair launch: fpd_conv_pair_fused_wgrad_partials (counts for p->a and p->b; returns 0 / error code). */
int fpd_conv_fused_wgrad_partials(const fpd_conv_t* a);
/* 1 if fpd_conv_forward() / fpd_conv_forward_pair() would serve these launches WITH a folded BN-backward apply (fold_x set
 * or not: only the dimensions, epilogue and prologue are looked at); 0 otherwise. */
int fpd_conv_fold_supported(const fpd_conv_t* a);
int fpd_conv_pair_fold_supported(const fpd_conv_pair_t* p);
/* The instantiation of the halo-tile kernel (csrc/conv_tile.hip) that would run this launch / pair launch, decided by the route
 * function the launch walks; the fold is asked for where fold_x is set.  Pure host code, nothing is dereferenced.
 *   element size (2 / 4) | BK << 4 | TN << 12 | ALLW << 16 | FOLD << 17,   or -1 where that kernel declines.
 * (Whether the dispatch reaches that kernel depends on the options "conv_c1" / "conv_c3" / "conv_pp" and the back end.) */
int fpd_conv_tile_variant(const fpd_conv_t* a);
int fpd_conv_tile_pair_variant(const fpd_conv_pair_t* p);
/* ... of wgrad_tile_kernel (csrc/wgrad_tile.hip) for this weight gradient, a->partial set or not as it will be launched:
 *   dtype | R << 4 | TP << 8 | H4 << 20 | SMALL << 21 | KSPLIT << 22,   or -1 where it declines or hands the launch to wgrad3. */
int fpd_wgrad_tile_variant(const fpd_wgrad_t* a);
/* 1 if fpd_conv_forward() would serve this launch WITH its second source (x2, w2, bias2, C2 filled in as they will be
 * launched); 0 otherwise.  Process-wide switch: FPD_FUSE_SKIP=0 / fpd_set_option("conv_skip", 0). */
int fpd_conv_skip_supported(const fpd_conv_t* a);
int fpd_conv_pair_fused_wgrad_partials(const fpd_conv_pair_t* p, int32_t* n_a, int32_t* n_b);
int fpd_conv_wgrad(const fpd_wgrad_t* a, fpd_stream_t stream);
int fpd_wgrad_num_partials(const fpd_wgrad_t* a);   /* slabs fpd_conv_wgrad writes when a->partial is set */
int fpd_wgrad_reduce(const fpd_wreduce_entry_t* table_dev, int32_t n_entries, int64_t max_elems, fpd_stream_t stream);
int fpd_stem_forward(const fpd_stem_t* a, fpd_stream_t stream);
/* 1 if fpd_stem_forward() would serve this launch WITH the eval-mode BN + ReLU of a->act in its epilogue; 0 otherwise.
 * Process-wide switch: FPD_STEM_ACT=0 / fpd_set_option("stem_act", 0). */
int fpd_stem_act_supported(const fpd_stem_t* a);
int fpd_stem_wgrad(const fpd_stem_t* a, fpd_stream_t stream);
int fpd_stem_wgrad_num_partials(const fpd_stem_t* a);   /* slabs fpd_stem_wgrad writes when a->partial is set */
int fpd_elementwise(const fpd_ew_t* a, fpd_stream_t stream);
/* two independent elementwise ops of the same kind in one launch (else one after the other) */
typedef struct { fpd_ew_t a, b; } fpd_ew_pair_t;
int fpd_elementwise_pair(const fpd_ew_pair_t* p, fpd_stream_t stream);
int fpd_loss(const fpd_loss_t* a, fpd_stream_t stream);
/* The launch fpd_loss() makes for `a` as it stands (pure host code: dimensions, dtype and the alignment of teacher, out[s] and
 * dout[s] are looked at, nothing is dereferenced).  vectorised: 1 = 16-byte vectors of joints, tiles of 128 pixels (J a multiple
 * of 8 in bf16, 4 in fp32, and every map 16-byte aligned), 0 = the element-per-thread kernel, tiles of 64 pixels.  blocks: the
 * grid = the number of terms added to each of losses[0..1].  tiles_per_block: tiles of one image a block walks (the last block
 * of an image may own fewer).  Returns 0, or the error code fpd_loss() would give for these dimensions. */
int fpd_loss_geometry(const fpd_loss_t* a, int32_t* vectorised, int32_t* blocks, int32_t* tiles_per_block);
int fpd_loss_ohkm(const fpd_loss_ohkm_t* a, fpd_stream_t stream);
/* bytes of fpd_loss_ohkm_t.scratch for these dimensions (B, J, H, W, S are looked at); negative on bad dimensions */
int64_t fpd_loss_ohkm_scratch_bytes(const fpd_loss_t* a);
int fpd_loss_kl(const fpd_loss_kl_t* a, fpd_stream_t stream);
/* bytes of fpd_loss_kl_t.scratch for these dimensions (B, J, H, W, S are looked at); negative on bad dimensions */
int64_t fpd_loss_kl_scratch_bytes(const fpd_loss_t* a);
int fpd_adam(const fpd_adam_t* a, fpd_stream_t stream);
int fpd_adamw(const fpd_adamw_t* a, fpd_stream_t stream);
/* The launch fpd_adamw() makes for `a` as it stands (pure host code, nothing is dereferenced).  blocks: its grid;
 * *vec_elems: the leading elements moved as 16-byte vectors (a multiple of 4; 0 = element by element).  Returns 0, or the
 * error code fpd_adamw() would give. */
int fpd_adamw_geometry(const fpd_adamw_t* a, int32_t* blocks, int64_t* vec_elems);
/* refuses (before any launch) null param / grad, n < 0, momentum < 0, weight_decay < 0, momentum != 0 without buf, nesterov without momentum */
int fpd_sgd(const fpd_sgd_t* a, fpd_stream_t stream);
int fpd_ema(const fpd_ema_t* a, fpd_stream_t stream);
/* The launch fpd_ema() makes for `a` as it stands (pure host code: counts and pointer alignments are looked at, nothing is
 * dereferenced).  blocks: the grid of the one kernel (256 threads a block; a thread walks a segment's vectors, then its
 * single elements, with a stride of 256 * blocks).  vec_elems[s], s < nseg: the leading elements of segment s moved as
 * 16-byte vectors (a multiple of 4; 0 = the element-by-element path).  Returns 0, or the error code fpd_ema() would give. */
int fpd_ema_geometry(const fpd_ema_t* a, int32_t* blocks, int64_t* vec_elems);
int fpd_grad_clip(const fpd_grad_clip_t* a, fpd_stream_t stream);
/* bytes of `partial` that serve n elements at any alignment of grad (8 per block of the largest grid); negative: n refused */
int64_t fpd_grad_clip_scratch_bytes(int64_t n);
/* The launches fpd_grad_clip() makes for `a` as it stands (pure host code, nothing is dereferenced).  blocks: the grid of the
 * sum and of the scale launch = the partials written; *vec_elems: the leading elements read as 16-byte vectors (a multiple
 * of 4; 0 = element by element).  Returns 0, or the error code fpd_grad_clip() would give. */
int fpd_grad_clip_geometry(const fpd_grad_clip_t* a, int32_t* blocks, int64_t* vec_elems);
int fpd_grad_accum(const fpd_grad_accum_t* a, fpd_stream_t stream);
/* The launch fpd_grad_accum() makes for `a` as it stands (pure host code, nothing is dereferenced).  blocks: its grid;
 * *vec_elems: the leading elements moved as 16-byte vectors (a multiple of 4; 0 = element by element).  Returns 0, or the
 * error code fpd_grad_accum() would give. */
int fpd_grad_accum_geometry(const fpd_grad_accum_t* a, int32_t* blocks, int64_t* vec_elems);
int fpd_weight_prep(const fpd_wprep_entry_t* table_dev, int32_t n_entries, int64_t max_elems, int32_t dtype,
                    fpd_stream_t stream);
int fpd_bn_update_running(const fpd_bnupd_entry_t* table_dev, int32_t n_entries, fpd_stream_t stream);
int fpd_cast(const void* src, void* dst, int64_t n, int32_t src_dtype, int32_t dst_dtype, fpd_stream_t stream);
/* [N,C,H,W] fp32 <-> [N,H,W,C] dtype layout changes at the module boundary */
int fpd_nchw_to_nhwc(const float* src, void* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t dtype,
                     fpd_stream_t stream);
int fpd_nhwc_to_nchw(const void* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t dtype,
                     fpd_stream_t stream);

/* Per-step training metric (lib/core/evaluate.py:16-71 accuracy, lib/core/inference.py:18-46 get_max_preds): heat-map
 * arg-max of prediction and target, PCK@thr over the batch, bit-exact with the reference (first maximum wins; the
 * normaliser is the reference's [h, w]/10 applied to (x, y), evaluate.py:55; float64 distances and averages).  One call
 * appends {avg_acc, cnt, pose_loss, kd_loss} (what the reference passes to its AverageMeters every iteration,
 * function.py:150-155) to the device log ring at slot *cursor % log_slots and advances the cursor -- no host
 * synchronisation; the host drains the ring when it prints a log line. */
typedef struct {
    int32_t B, J, H, W, dtype, log_slots;
    float thr;             /* 0.5 in the reference */
    int32_t _pad;
    const void* out;       /* prediction [B,H,W,J] (NHWC, dtype) */
    const float* target;   /* [B,J,H,W] fp32 (NCHW, as the loader delivers it) */
    float* counts;         /* [J][2] workspace {hits, valid}, zero on entry, zeroed again on exit */
    double* log;           /* [log_slots][4] {avg_acc, cnt, pose, kd} */
    long long* cursor;     /* device counter of appended entries */
    const double* losses;  /* optional [2] {pose, kd} of this iteration (fpd_loss_t.losses), copied into the log entry */
} fpd_pck_t;
int fpd_pck(const fpd_pck_t* a, fpd_stream_t stream);

/* ---- fp8 (OCP e4m3fn) forward convolutions on the CDNA4 fp8 matrix pipe: BASELINE configs[4] "HRNet-W32 student fp8
 * weights (CDNA4 fp8 MFMA)" ---- */
/* fpd_conv_forward() with e4m3 weights: `c` is the convolution exactly as fpd_conv_t describes it (c.w = the bf16
 * working weights, used when the shape is outside the fp8 kernel's domain); w8 = the same weights as e4m3 bytes
 * [K][R][S][C], w8_scale[k] = the fp32 scale of output channel k (w ~= w8 * scale).  The activation operand (after the
 * fused BN+ReLU prologue) is rounded to e4m3 at unit scale, saturating at +-448, on its way into LDS; products
 * accumulate in fp32 (v_mfma_f32_32x32x16_fp8_fp8); scale, bias, residual and the batch statistics follow in fp32.
 * Domain of the fp8 kernel: dtype BF16, plain epilogue, stride-1 "same" 1x1/3x3, W <= 128, C % 32 == 0, K % 8 == 0. */
typedef struct {
    fpd_conv_t c;
    const void* w8;
    const float* w8_scale;
} fpd_conv_f8_t;
int fpd_conv_forward_f8(const fpd_conv_f8_t* a, fpd_stream_t stream);
int fpd_conv_f8_in_domain(const fpd_conv_t* c);   /* 1 = the fp8 kernel takes this shape, 0 = falls back to c.w */
/* The instantiation of the fp8 kernel (csrc/conv_tile_f8.hip, compiled for TN in {1, 2, 4} accumulator tiles of 32 output
 * channels x BK in {32, 64} channels a chunk) that would run this launch, decided by the route function the launch walks.
 * Pure host code, nothing is dereferenced.   TN | BK << 4,   or -1 exactly where fpd_conv_f8_in_domain() is 0. */
int fpd_conv_f8_variant(const fpd_conv_t* a);

/* fp32 master weights -> e4m3 + per-output-channel scale (amax / 448; 1 for an all-zero row), one launch for a table. */
typedef struct {
    const float* w;        /* [K][RSC] fp32 master weights (K,R,S,C order) */
    void* w8;              /* [K][RSC] e4m3 bytes */
    float* scale;          /* [K] */
    int32_t K, RSC;
} fpd_wquant_entry_t;
int fpd_weight_quant_f8(const fpd_wquant_entry_t* table_dev, int32_t n_entries, fpd_stream_t stream);

/* ---- validate / flip-test post-processing (lib/core/function.py:189-332) ---- */
/* y[r][c] = x[r][W-1-c] for `rows` rows of W floats: the flipped input image of the flip test
 * (function.py:217-221: np.flip(input.cpu().numpy(), 3)); x is [N,3,H,W] fp32, rows = N*3*H. */
int fpd_flip_w(const float* x, float* y, int64_t rows, int32_t W, fpd_stream_t stream);

/* flip_back (lib/utils/transforms.py:15-29) + the one-pixel shift of the flipped map (function.py:233-236,
 * TEST.SHIFT_HEATMAP) + the average (function.py:238) in one pass over fp32 [N,J,H,W] maps:
 *   f[n,j,y,x]  = b[n, src[j], y, W-1-x]               (width reversed, left/right joint channels swapped)
 *   f'[.., x]   = shift && x >= 1 ? f[.., x-1] : f[.., x]
 *   y           = (a + f') * 0.5f
 * src[j] is the channel of b that lands in channel j after flip_back's sequential pair swaps. */
#define FPD_MAX_JOINTS 32
typedef struct {
    int32_t N, J, H, W;
    int32_t shift, _pad;
    const float* a;        /* [N,J,H,W] model(input)[-1]; NULL: y = f' (flip_back + shift only, no average) */
    const float* b;        /* [N,J,H,W] model(flipped input)[-1] */
    float* y;              /* [N,J,H,W] (may alias a, not b) */
    int32_t src[FPD_MAX_JOINTS];
} fpd_flipmerge_t;
int fpd_flip_merge(const fpd_flipmerge_t* a, fpd_stream_t stream);

/* get_final_preds (lib/core/inference.py:49-79): per (sample, joint) the heat-map arg-max (first maximum wins;
 * coordinates zeroed where the maximum is not positive, inference.py:18-46), the quarter-pixel shift towards the higher
 * neighbour when post_process (TEST.POST_PROCESS, inference.py:57-70) and transform_preds (lib/utils/transforms.py:50-55):
 * preds = trans[n] . [x, y, 1] in float64, stored as float32.  trans[n] is the 2x3 inverse affine of sample n
 * (get_affine_transform(center, scale, 0, [W, H], inv=1), transforms.py:57-92 -- six doubles per sample computed by
 * the caller); trans/preds NULL = heat-map coordinates only. */
typedef struct {
    int32_t N, J, H, W;
    int32_t post_process, _pad;
    const float* hm;       /* [N,J,H,W] fp32 */
    const double* trans;   /* [N][2][3] or NULL */
    float* coords;         /* [N,J,2] heat-map coordinates (x, y) after post-processing */
    float* preds;          /* [N,J,2] image coordinates, or NULL */
    float* maxvals;        /* [N,J] */
} fpd_finalpreds_t;
int fpd_final_preds(const fpd_finalpreds_t* a, fpd_stream_t stream);

/* The post-processing of one validation batch in ONE launch, reading the network's last map where it lies in the arena
 * (NHWC) and writing straight into the device-resident result arrays of the whole validation -- what
 * fpd_nhwc_to_nchw x 2 + fpd_flip_merge + fpd_nchw_to_nhwc + a host loop of get_affine_transform + fpd_final_preds did:
 *   merged[n,y,x,j] = b ? (a[n,y,x,j] + f'[n,y,x,j]) * 0.5f : (float)a[n,y,x,j]        (f' as in fpd_flipmerge_t, fp32)
 *   all_preds[row0+n, j] = {x, y, maxval}: arg-max, zeroing and quarter-pixel shift of final_preds on `merged`, mapped by
 *                          get_affine_transform(center[n], scale[n], 0, [W, H], inv=1) computed on the device in
 *                          numpy's dtypes and operation order (csrc/val_post_math.h), float64 product stored as float32
 *   all_boxes[row0+n]    = {center, scale, prod(scale * 200), score} in float64
 * Bit-identical to that chain.  Rows outside [row0, row0+N) are not touched.  Refused before any launch: null pointers,
 * J > FPD_MAX_JOINTS, merged aliasing a or b, row0 < 0, row0 + N > rows. */
typedef struct {
    int32_t N, J, H, W;
    int32_t dtype;                 /* of a and b: FPD_F32 or FPD_BF16 */
    int32_t shift, post_process;   /* TEST.SHIFT_HEATMAP (only with b), TEST.POST_PROCESS */
    int32_t box_f32;               /* 1: center/scale hold float32 values (fpd_aug_db_t.box_f32): scale * 200 stays float32 */
    int64_t row0;                  /* first result row of this batch */
    int64_t rows;                  /* rows all_preds / all_boxes hold: row0 + N <= rows */
    const void* a;                 /* [N,H,W,J] last map of the network for the batch */
    const void* b;                 /* the same for the width-flipped batch, or NULL: no flip test */
    const double* center;          /* [N,2] device */
    const double* scale;           /* [N,2] device */
    const double* score;           /* [N] device */
    float* merged;                 /* [N,H,W,J] fp32 (what fpd_loss with S = 1 and fpd_pck read) */
    float* all_preds;              /* [rows,J,3] float32 */
    double* all_boxes;             /* [rows,6] float64 */
    int32_t src[FPD_MAX_JOINTS];   /* as in fpd_flipmerge_t */
} fpd_val_post_t;
int fpd_val_post(const fpd_val_post_t* a, fpd_stream_t stream);

/* Distribution-aware coordinate decoding (DARK, Zhang et al., CVPR 2020) in place of the quarter-pixel shift, one launch,
 * per (sample, joint) with m the fp32 map (csrc/dark.hip, the Newton step in csrc/dark_math.h):
 *   arg-max as in fpd_final_preds (first maximum wins, (0, 0) where the maximum is not positive); maxval from the raw map
 *   B  = the separable blur of m with taps[ksize], rows then columns, zeros outside the map
 *   L  = log(max(B * (maxval / max(B)), 1e-10)); nothing is refined where maxval <= 0 or max(B) <= 0
 *   where 1 < px < W - 2 and 1 < py < H - 2: (x, y) += -Hess(L)^-1 grad(L) by central differences, if det(Hess) != 0,
 *   in float64, rounded once into the float32 coordinate
 * then the map to image coordinates in one of two forms:
 *   (a) trans / preds as in fpd_finalpreds_t (both NULL: heat-map coordinates only)
 *   (b) center / scale / box_f32 / row0 / rows / all_preds as in fpd_val_post_t: ONLY x and y of rows row0 .. row0+N-1 of
 *       all_preds are written; maxval and all_boxes stay what fpd_val_post (post_process = 0) wrote
 * taps: the normalised Gaussian of OpenCV's getGaussianKernel(ksize, 0), ksize odd in [9, 31], computed by the caller in
 * float64.  Refused before any launch: null hm or taps, bad ksize or layout, J > FPD_MAX_JOINTS, H * W > FPD_DARK_MAX_HW
 * (two fp32 images of the map live in LDS), both or neither of (a) and (b) other than the coordinates-only form,
 * row0 < 0, row0 + N > rows. */
#define FPD_DARK_NCHW 0
#define FPD_DARK_NHWC 1
#define FPD_DARK_MIN_KSIZE 9
#define FPD_DARK_MAX_KSIZE 31
#define FPD_DARK_MAX_HW 16384
typedef struct {
    int32_t N, J, H, W;
    int32_t layout, ksize;         /* FPD_DARK_NCHW: [N,J,H,W] (the module API's output); FPD_DARK_NHWC: [N,H,W,J] (`merged`) */
    int32_t box_f32, _pad;         /* form (b), as in fpd_val_post_t */
    int64_t row0, rows;            /* form (b) */
    const float* hm;               /* fp32 map in `layout` */
    const double* taps;            /* [ksize] device */
    float* coords;                 /* [N,J,2] heat-map coordinates (x, y), or NULL */
    float* maxvals;                /* [N,J], or NULL */
    int32_t* refined;              /* [N,J] 1 where the Newton step was taken (a zero step included), or NULL */
    const double* trans;           /* (a) [N][2][3] */
    float* preds;                  /* (a) [N,J,2] image coordinates */
    const double* center;          /* (b) [N,2] device */
    const double* scale;           /* (b) [N,2] device */
    float* all_preds;              /* (b) [rows,J,3] float32: x and y of the batch's rows are overwritten */
} fpd_dark_t;
int fpd_dark_refine(const fpd_dark_t* a, fpd_stream_t stream);

/* ---- debug images (lib/utils/vis.py of the reference: save_batch_image_with_joints, save_batch_heatmaps) ---- */
/* The canvases the reference composes on the host with torchvision, cv2 and numpy, rendered on the device from the tensors
 * of the iteration; per-pixel arithmetic in csrc/vis_math.h.  The caller owns every buffer, downloads the uint8 canvases
 * and encodes them.  Nothing here synchronises.  Heat maps come in one of three forms:
 *   layout FPD_VIS_NCHW, dtype FPD_F32             the loader's target
 *   layout FPD_VIS_NHWC, dtype FPD_F32 / FPD_BF16  a merged validation map / a network's last map where it lies in the arena */
#define FPD_VIS_NCHW 0
#define FPD_VIS_NHWC 1

/* out[0] = min, out[1] = max of n float32 values (exact: no rounding is involved; -0 counts as 0). */
typedef struct {
    int64_t n;
    const float* x;
    float* out;            /* float[2], device */
} fpd_vis_minmax_t;
int fpd_vis_minmax(const fpd_vis_minmax_t* a, fpd_stream_t stream);

/* get_max_preds (lib/core/inference.py:18-46): per (sample, joint) the arg-max of the map (first maximum wins) as
 * (x, y) = (idx % w, idx / w), zeroed where the maximum is <= 0, and the maximum itself. */
typedef struct {
    int32_t N, J, h, w;
    int32_t dtype, layout;
    const void* hm;
    float* preds;          /* [N,J,2] */
    float* maxvals;        /* [N,J] */
} fpd_vis_max_preds_t;
int fpd_vis_max_preds(const fpd_vis_max_preds_t* a, fpd_stream_t stream);

/* save_batch_image_with_joints up to the file write: make_grid(image, nrow, padding, normalize=True) as bytes,
 *   xmaps = min(nrow, N), ymaps = ceil(N / xmaps), canvas [(H+padding)*ymaps+padding, (W+padding)*xmaps+padding, 3],
 *   cell k at (k / xmaps * (H+padding) + padding, k % xmaps * (W+padding) + padding), everything else 0;
 *   N == 1: the canvas is the bare [H, W, 3] image (make_grid returns it unpadded) and the marks keep the +padding offset;
 *   byte = trunc(clamp(((x + float32(-min)) / float32(double(max) - double(min) + 1e-5)) * 255, 0, 255)) in float32;
 * the tensor's channels in positions 0, 1, 2.  Then for every joint with vis != 0 the pixels 1 <= dx^2 + dy^2 <= 9 around
 *   (int(cx * (W+padding) + padding + jx * coord_scale), int(cy * (H+padding) + padding + jy * coord_scale))   (float64 sums)
 * are set to (255, 0, 0), clipped to the canvas (a compose launch, then a scatter launch: every mark stores one value). */
typedef struct {
    int32_t N, H, W, J;
    int32_t nrow, padding;
    int32_t joints_f64;            /* joints hold float64 (1) or float32 (0) */
    int32_t joints_stride;         /* elements per joint (>= 2): x, y first */
    float coord_scale;
    int32_t _pad;
    int64_t canvas_bytes;          /* size of canvas: must be GH * GW * 3 */
    const float* image;            /* [N,3,H,W] */
    const float* minmax;           /* fpd_vis_minmax of the image */
    const void* joints;            /* [N,J,joints_stride] */
    const float* vis;              /* [N,J] */
    uint8_t* canvas;               /* [GH,GW,3] */
} fpd_vis_joints_grid_t;
int fpd_vis_joints_grid(const fpd_vis_joints_grid_t* a, fpd_stream_t stream);

/* save_batch_heatmaps up to the file write: canvas [N*h, (J+1)*w, 3] from image [N,3,H,W] with H == 4*h, W == 4*w.
 *   resized = (a + b + c + d + 2) >> 2 over rows / columns 4i+1, 4i+2 of the byte image (normalize: as above; else x itself)
 *   mark(k) = the four pixels dx^2 + dy^2 == 1 around (int(preds[n,k,0]), int(preds[n,k,1])), clipped to the tile
 *   tile 0   = resized, (0,0,255) at the marks of all joints
 *   tile j+1 = trunc(table[heat byte] * 0.7 + base * 0.3) in float64, base = resized with (0,0,255) at the marks of joints
 *              0..j; then (0,0,255) at mark(j).  heat byte = trunc(clamp(float32(m) * 255, 0, 255)). */
typedef struct {
    int32_t N, J, h, w, H, W;
    int32_t dtype, layout;         /* of hm */
    int32_t normalize, _pad;
    int64_t canvas_bytes;          /* must be N*h * (J+1)*w * 3 */
    const float* image;            /* [N,3,H,W] */
    const float* minmax;           /* fpd_vis_minmax of the image; may be NULL when normalize == 0 */
    const void* hm;
    const float* preds;            /* [N,J,2] of fpd_vis_max_preds */
    const uint8_t* table;          /* [256,3] colour of every heat byte */
    uint8_t* canvas;
} fpd_vis_heatmap_grid_t;
int fpd_vis_heatmap_grid(const fpd_vis_heatmap_grid_t* a, fpd_stream_t stream);

/* ---- device data pipeline (lib/dataset/JointsDataset.py:113-198,233-289) ---- */
/* generate_target (JointsDataset.py:233-289) for a batch: Gaussian heat-map targets + target weights from joint
 * positions in network-input pixels.  mu = int(joint / feat_stride + 0.5) in float64 (feat_stride = image/heat-map size),
 * the (6*sigma+1)^2 patch `g` (built once by the caller with the reference's float32 numpy expression, so the values are
 * the reference's bit for bit) is pasted clipped at the border when weight > 0.5; weight = 0 when the patch lies fully
 * outside.  Index work is bit-exact with the reference. */
typedef struct {
    int32_t B, J, H, W;            /* heat-map shape */
    int32_t patch, _pad;           /* patch edge = 6*sigma + 1 */
    double stride_x, stride_y;     /* image_size / heatmap_size */
    const double* joints;          /* [B,J,3] (x, y, -) in network-input pixels */
    const float* vis;              /* [B,J] joints_vis[:, 0] */
    const float* g;                /* [patch][patch] */
    float* target;                 /* [B,J,H,W] */
    float* weight;                 /* [B,J] */
} fpd_targets_t;
int fpd_render_targets(const fpd_targets_t* a, fpd_stream_t stream);

/* DARK's unbiased target encoding (Zhang et al., CVPR 2020: generate_target / adjust_target_weight of the published code):
 * the Gaussian is evaluated at the real-valued joint position over the whole map, so that a network trained on these
 * targets predicts sub-pixel peaks, which fpd_dark_refine then recovers.  fpd_render_targets rounds the centre to a pixel
 * first, and the best decode of such a map is that pixel.
 *
 * UNPINNED: the DarkPose source is not available to this project.  The text below is the definition; it restates the
 * published rule in this project's terms and has not been compared with a run of the authors' code.
 *
 * For every (sample b, joint j), tmp = 3 * sigma, all arithmetic in float64 unless noted:
 *   mu_x = joints[b,j,0] / stride_x, mu_y = joints[b,j,1] / stride_y        one division each, no + 0.5, no rounding
 *   ulx = (int)(mu_x - tmp), brx = (int)(mu_x + tmp + 1); uly, bry likewise from mu_y.  The cast truncates toward zero like
 *         Python's int() (so it is not a floor below zero)
 *   outside = ulx >= W || uly >= H || brx < 0 || bry < 0; a centre that is not finite is outside as well (Python's int()
 *         raises there)
 *   w = outside ? 0 : vis[b,j]
 *   weight[b,j] = w * joints_weight[j] as a float32 product; joints_weight NULL: w (as in fpd_render_targets_w)
 *   !outside && w > 0.5f: EVERY pixel (x, y) of the H x W map is (float)exp(-((x - mu_x)^2 + (y - mu_y)^2) / (2 sigma^2)),
 *         evaluated in float64 and rounded once to float32.  There is no patch window.
 *   otherwise the whole map is +0.0f.
 * Tolerance of a written value against numpy's float32(exp(float64 expression)), derived, not measured: a float64
 * evaluation with a relative error below 2^-30 lands within 1 float32 ulp, which covers a direct exp and the separable
 * product ex[x] * ey[y] of two float64 factors that the kernel forms; where the exact value is below float32's smallest
 * normal (2^-126) an absolute 2^-126 is allowed (the factors may underflow to zero).  Weights and all-zero maps are exact.
 * H + W <= 8192 (the row and column factors live in LDS). */
typedef struct {
    int32_t B, J, H, W;            /* heat-map shape */
    int32_t sigma, _pad;           /* >= 1 */
    double stride_x, stride_y;     /* image_size / heatmap_size */
    const double* joints;          /* [B,J,3] (x, y, -) in network-input pixels */
    const float* vis;              /* [B,J] */
    const float* joints_weight;    /* [J] or NULL */
    float* target;                 /* [B,J,H,W] */
    float* weight;                 /* [B,J] */
} fpd_targets_unbiased_t;
int fpd_render_targets_unbiased(const fpd_targets_unbiased_t* a, fpd_stream_t stream);

/* The crop of JointsDataset.__getitem__ (:160-168) for a batch: cv2.warpAffine(img, trans, (W,H), INTER_LINEAR)
 * (constant zero border) -> ToTensor (/255, HWC->CHW) -> Normalize(mean, std) (tools/fpd_train.py:182-193), one pass,
 * reading interleaved 8-bit source images that differ in size.  The bilinear sample follows OpenCV's fixed-point scheme
 * (source coordinates in 1/32 pixel from 10-bit fixed-point row/column terms, 15-bit weights, 8-bit rounded result)
 * so that the 8-bit intermediate matches cv2's; `minv` is the DST->SRC map (the inverse of get_affine_transform's
 * matrix, what cv2.warpAffine computes internally with invertAffineTransform). */
typedef struct {
    const uint8_t* img;            /* [h][w][3] interleaved */
    int32_t h, w;
    int64_t row_bytes;
    double minv[6];
} fpd_warp_src_t;
typedef struct {
    int32_t B, H, W, _pad;         /* output [B,3,H,W] fp32 */
    const fpd_warp_src_t* src;     /* device table [B] */
    float mean[3], std[3];         /* ToTensor + Normalize in torch's fp32 order: (u8 / 255.f - mean) / std, per SOURCE channel */
    float* out;
} fpd_warp_t;
int fpd_warp_affine(const fpd_warp_t* a, fpd_stream_t stream);

/* ---- on-device training augmentation (JointsDataset.py:137-179, utils/transforms.py:32-110) ----
 * Everything __getitem__ does after the image is decoded, as three launches per batch with no host work per sample:
 * fpd_augment_params -> fpd_warp_affine_aug -> fpd_render_targets_w.  The dataset lives on the device (fpd_aug_db_t). */
typedef struct {
    const uint8_t* img;            /* [h][w][3] interleaved, anywhere in one packed device buffer */
    int32_t h, w;
    int64_t row_bytes;
} fpd_aug_img_t;
typedef struct {
    int32_t N, J;                  /* images / joints per image (J <= 64) */
    int32_t box_f32, _pad;         /* 1: center/scale hold float32 values (COCO's _box2cs); numpy then keeps the flipped
                                      centre and the validation-mode scale*200 in float32 */
    const fpd_aug_img_t* images;   /* [N] */
    const double* joints;          /* [N,J,3] image pixels */
    const float* vis;              /* [N,J] joints_3d_vis[:, 0] */
    const double* center;          /* [N,2] */
    const double* scale;           /* [N,2] */
    const int32_t* flip_src;       /* [J]: joint that ends up at j after fliplr_joints' sequential pair swaps */
    const int32_t* upper;          /* [J]: 1 = joint id in upper_body_ids */
    double aspect_ratio;           /* image width / height (a Python float in the reference: enters float32 arithmetic) */
    double pixel_std;              /* 200 */
} fpd_aug_db_t;
/* What fpd_augment_params hands to the crop, per sample. */
typedef struct {
    int32_t src;                   /* index into fpd_aug_db_t.images; -1 = index out of range (the crop reads nothing) */
    int32_t flip;                  /* 1: tap column X reads source column w-1-X (the mirrored image, not a composed matrix) */
    double minv[6];                /* DST->SRC map, invertAffineTransform of `trans` */
} fpd_aug_crop_t;
/* Draw table columns (what the reference pulls from np.random / random per sample, in its order of use):
 *   0 u_half  rand()  < prob_half_body          1 n_half  randn() < 0.5: upper body
 *   2 n_scale randn() scale jitter              3 n_rot   randn() rotation jitter
 *   4 u_rot   random() <= 0.6: rotate           5 u_flip  random() <= 0.5: flip
 * idx / draws are strided so that both can live in one [B,8]-double staging row (int32 index in the first word). */
typedef struct {
    fpd_aug_db_t db;
    int32_t B, is_train;           /* is_train 0: draws ignored, r = 0, no flip, no half-body */
    int32_t flip, num_joints_half_body;
    int32_t idx_stride, draw_stride;    /* in int32 / in doubles */
    int32_t out_w, out_h;          /* cfg.MODEL.IMAGE_SIZE */
    double sf, rf, prob_half_body;
    const int32_t* idx;            /* [B] sample -> image */
    const double* draws;           /* [B][>=6] */
    fpd_aug_crop_t* crop;          /* [B] */
    double* trans;                 /* [B,2,3] SRC->DST, get_affine_transform(c, s, r, image_size) */
    double* joints;                /* [B,J,3] transformed (visible joints), third column 0 */
    float* vis;                    /* [B,J] after the flip's exchange */
    double* center;                /* [B,2] */
    double* scale;                 /* [B,2] */
    double* rotation;              /* [B] degrees */
    int32_t* flipped;              /* [B] */
} fpd_augment_t;
int fpd_augment_params(const fpd_augment_t* a, fpd_stream_t stream);

/* fpd_warp_affine reading its per-sample source, matrix and flip flag from what fpd_augment_params wrote. */
typedef struct {
    int32_t B, H, W, N;            /* output [B,3,H,W] fp32; N images in the table */
    const fpd_aug_img_t* images;   /* [N] */
    const fpd_aug_crop_t* crop;    /* [B] */
    float mean[3], std[3];
    float* out;
} fpd_warp_aug_t;
int fpd_warp_affine_aug(const fpd_warp_aug_t* a, fpd_stream_t stream);

/* fpd_render_targets with JointsDataset.py:286-287: the written weight is vis_or_zero * joints_weight[j] (float32); the
 * paste decision uses the unmultiplied weight.  joints_weight NULL = fpd_render_targets. */
typedef struct {
    fpd_targets_t t;
    const float* joints_weight;    /* [J] or NULL */
} fpd_targets_w_t;
int fpd_render_targets_w(const fpd_targets_w_t* a, fpd_stream_t stream);

/* ---- rescoring + OKS NMS of COCO's evaluate (coco.py:334-369, nms/nms.py:75-177): every picture in one launch ----
 * One workgroup owns a picture (grid-stride over pictures when `grid` caps the launch) and runs the greedy loop itself; any
 * number of people per picture.  The people of picture i are rows offsets[i] .. offsets[i+1] of the per-person arrays.
 *   score[p] = mean of the maxvals > (float)in_vis_thre (float32, summed in joint order; 0 without any) * box_score[p]
 *              (float64); rescore 0: score[p] = box_score[p] as it is (nms.oks_nms gets rescored people)
 *   oks(g,d) = mean_j exp(-((xd-xg)^2 + (yd-yg)^2 [float32] / (2 sigma_j)^2 / ((area_g + area_d)/2 + 2^-52) / 2)) [float64]
 *   hard (soft 0): pick the highest score, drop everyone left with oks > oks_thre, repeat
 *   soft (soft 1): at most 20 picks; after each the working scores of the rest become s * exp(-oks^2 / oks_thre)
 * Equal (working) scores: the lower index is picked first.  keep holds, per picture, the picked people as indices local to
 * the picture in pick order, -1 in the remaining slots; n_keep[i] their number, or -1 if offsets[i..i+1] do not describe a
 * range inside [0, P_total] (nothing of that picture is then read or written). */
typedef struct {
    int32_t P_total, n_img;        /* people over all pictures / pictures */
    int32_t J;                     /* joints per person, 1..64 */
    int32_t soft, rescore;         /* 0 / 1 each */
    int32_t grid;                  /* workgroups launched; 0 = min(n_img, 4096) */
    double in_vis_thre, oks_thre;
    const float* kpts;             /* [P_total,J,3] x, y, maxval */
    const double* area;            /* [P_total] */
    const double* box_score;       /* [P_total] */
    const int32_t* offsets;        /* [n_img+1] */
    const double* sigmas;          /* [J] */
    double* score;                 /* [P_total] out */
    double* work;                  /* [P_total] scratch: the working scores */
    int32_t* keep;                 /* [P_total] out */
    int32_t* n_keep;               /* [n_img] out */
    double* oks_first;             /* [P_total] or NULL: oks of every person (the pick itself included) with the first pick of its picture */
} fpd_oks_nms_t;
int fpd_oks_nms(const fpd_oks_nms_t* a, fpd_stream_t stream);

/* ---- COCO keypoint AP (lib/dataset/coco_eval.py): OKS matrix + greedy matching of every picture in one launch ----
 * One workgroup owns a picture (grid-stride over pictures when `grid` caps the launch).  The gts of picture i are rows
 * gt_offsets[i] .. gt_offsets[i+1] of the gt arrays, its detections (best score first, the host cuts them to the 20 best) rows
 * dt_offsets[i] .. dt_offsets[i+1]; its OKS matrix [D_i, G_i] starts at oks[oks_offsets[i]].  Any number of either.
 *   oks[d,g]  = mean over the gt's annotated joints (v > 0) of exp(-e_j) -- float64, no contraction, summed in joint order --
 *                 e_j = ((xd-xg)^2 + (yd-yg)^2) / (2 sigma_j)^2 / (area_g + 2^-52) / 2
 *               a gt without an annotated joint: over every joint, with dx = max(0, x0 - xd) + max(0, xd - x1) (dy alike),
 *                 [x0, x1] = [bx - bw, bx + 2 bw] the gt box doubled about itself
 *   dt_area[d] = (max x - min x) * (max y - min y) over the detection's joints
 *   for each area range r (area_lo[r] .. area_hi[r], both ends inside) and threshold t = oks_thrs[k], independently:
 *     a gt is ignored when bit 0 of its flags is set or its area lies outside the range; gt_counted[r] counts the others
 *     the detections in order: best = min(t, 1 - 1e-10); first over the counting gts in their order, then -- only if none
 *     matched -- over the ignored ones: skip a gt already taken unless bit 1 of its flags (crowd) is set; skip oks < best;
 *     otherwise best = oks and the gt is the candidate (a tie goes to the later gt).  A candidate: matched = 1, dt_ignored = the
 *     gt is ignored, the gt is taken.  None: matched = 0, dt_ignored = dt_area[d] outside the range.
 * status[i] = 0, or -1 if an offset of picture i does not describe a range inside its array (nothing of that picture is then
 * read or written).  scratch: 31 bytes per gt (the ignore bits and, per (range, threshold), the taken flags of pictures with more
 * than 64 gts; smaller pictures keep both in registers / LDS). */
#define FPD_COCO_AREAS 3
#define FPD_COCO_THRS 10
typedef struct {
    int32_t n_img, J;              /* pictures / joints per person, 1..64 */
    int32_t G_total, D_total;      /* gts / detections over all pictures */
    int32_t grid, _pad;            /* workgroups launched; 0 = min(n_img, 8192) */
    int64_t oks_total;             /* elements of oks: the sum of D_i * G_i */
    double area_lo[FPD_COCO_AREAS], area_hi[FPD_COCO_AREAS];
    double oks_thrs[FPD_COCO_THRS];
    const double* gt_kpts;         /* [G_total,J,3] x, y, v */
    const double* gt_area;         /* [G_total] */
    const double* gt_bbox;         /* [G_total,4] x, y, w, h */
    const uint8_t* gt_flags;       /* [G_total] bit 0: ignore (crowd or no annotated joint), bit 1: crowd */
    const double* dt_kpts;         /* [D_total,J,3] */
    const int32_t* gt_offsets;     /* [n_img+1] */
    const int32_t* dt_offsets;     /* [n_img+1] */
    const int64_t* oks_offsets;    /* [n_img+1] */
    const double* sigmas;          /* [J] */
    double* oks;                   /* [oks_total] out */
    uint8_t* scratch;              /* [31,G_total] */
    uint8_t* matched;              /* [3,10,D_total] out */
    uint8_t* dt_ignored;           /* [3,10,D_total] out */
    int32_t* gt_counted;           /* [3,n_img] out */
    double* dt_area;               /* [D_total] out */
    int32_t* status;               /* [n_img] out */
} fpd_coco_match_t;
int fpd_coco_match(const fpd_coco_match_t* a, fpd_stream_t stream);

/* The precision / recall tables of those flags: one workgroup per (area range, threshold).  order[i] = the detection at rank i
 * of the stable descending sort of the scores; per rank tp = the running count of matched & ~ignored, fp of ~matched & ~ignored;
 *   rc = tp / npig[r], pr = tp / (fp + tp + 2^-52) made non-increasing from the right (suffix maximum);
 *   precision[k][q][r] = pr at the leftmost rank with rc >= rec_thrs[q], 0 past the end; recall[k][r] = the last rc, 0 without
 *   detections; both -1 where npig[r] == 0.
 * Counts are integers and a maximum is exact: equal flags give tables bit-equal to coco_eval.accumulate's.
 * status[r*10+k] = 0, or -1 if `order` held an index outside [0, D_total) (such a rank counts as ignored). */
typedef struct {
    int32_t D_total, n_rec;        /* detections / recall thresholds, 1..1024 */
    const uint8_t* matched;        /* [3,10,D_total] */
    const uint8_t* dt_ignored;     /* [3,10,D_total] */
    const int32_t* order;          /* [D_total] */
    const int32_t* npig;           /* [3] */
    const double* rec_thrs;        /* [n_rec] rising */
    int32_t* tp;                   /* [3,10,D_total] scratch: tp per rank */
    double* env;                   /* [3,10,D_total] scratch: pr, then its envelope */
    double* precision;             /* [10,n_rec,3] out */
    double* recall;                /* [10,3] out */
    int32_t* status;               /* [30] out */
} fpd_coco_accum_t;
int fpd_coco_accumulate(const fpd_coco_accum_t* a, fpd_stream_t stream);

/* ---- execution plan: a recorded list of the ops above, replayed with one call ---- */
enum {
    FPD_OP_CONV = 0, FPD_OP_WGRAD = 1, FPD_OP_STEM_FWD = 2, FPD_OP_STEM_WGRAD = 3, FPD_OP_EW = 4,
    FPD_OP_LOSS = 5, FPD_OP_ADAM = 6, FPD_OP_MEMSET = 7, FPD_OP_WPREP = 8, FPD_OP_BNUPD = 9, FPD_OP_WREDUCE = 10,
    FPD_OP_BNECK = 11, FPD_OP_BNECK_FOLD = 12, FPD_OP_CONV_PAIR = 13, FPD_OP_BNECK_PAIR = 14, FPD_OP_EW_PAIR = 15, FPD_OP_PCK = 16, FPD_OP_HEAD = 17,
    FPD_OP_HEAD_FOLD = 18, FPD_OP_NOP = 19, FPD_OP_AFFSUM = 20, FPD_OP_NCHW2NHWC = 21, FPD_OP_CONV_F8 = 22,
    FPD_OP_WQUANT = 23,         /* args: fpd_table_t over fpd_wquant_entry_t */
    FPD_OP_LOSS_OHKM = 24,      /* args: fpd_loss_ohkm_t */
    FPD_OP_SGD = 25,            /* args: fpd_sgd_t */
    FPD_OP_EW_MERGE = 26,       /* args: fpd_ew_merge_t */
    FPD_OP_LOSS_KL = 27,        /* args: fpd_loss_kl_t */
    FPD_OP_EMA = 28,            /* args: fpd_ema_t */
    FPD_OP_GRAD_CLIP = 29,      /* args: fpd_grad_clip_t */
    FPD_OP_GRAD_ACCUM = 30,     /* args: fpd_grad_accum_t */
    FPD_OP_ADAMW = 31           /* args: fpd_adamw_t */
};
typedef struct { void* ptr; int64_t bytes; } fpd_memset_t;                 /* zero-fill */
typedef struct { const void* table; int32_t n; int32_t dtype; int64_t max_elems; } fpd_table_t;

typedef struct fpd_plan fpd_plan;
fpd_plan* fpd_plan_create(void);
void fpd_plan_destroy(fpd_plan* p);
/* appends one op (args are copied); returns its index or <0 */
int fpd_plan_add(fpd_plan* p, int32_t op, const void* args, int64_t args_bytes);
int fpd_plan_size(const fpd_plan* p);
/* multi-lane schedule: op `op` is issued on lane `lane` (0 = the stream passed to run/capture, >0 = a stream owned
 * by the plan) after the ops listed in wait_ops[0..n_waits) (indices of ops on OTHER lanes) have completed; ops of
 * one lane execute in plan order.  Every fpd_plan_run/capture range forks the side lanes from `stream` at its start
 * and joins them back into `stream` at its end, so waits never need to cross a range boundary (such entries are
 * ignored).  Default for every op: lane 0, no waits = the plain in-order list. */
#define FPD_MAX_LANES 16
int fpd_plan_set_schedule(fpd_plan* p, int32_t op, int32_t lane, const int32_t* wait_ops, int32_t n_waits);
/* Hand-off to streams OUTSIDE the plan (the RCCL gradient all-reduce of one bucket, issued while the rest of the
 * backward still runs): fpd_plan_mark_event() asks fpd_plan_run() to record an event after op `op` each time it issues
 * it; fpd_plan_wait_op() makes `stream` wait for the most recent such record (hipStreamWaitEvent; no host sync).
 * FPD_OP_NOP (args: fpd_memset_t, ignored) launches nothing -- a pure ordering point in a lane. */
int fpd_plan_mark_event(fpd_plan* p, int32_t op);
int fpd_plan_wait_op(fpd_plan* p, int32_t op, fpd_stream_t stream);
/* launch ops [begin,end) on stream (and the plan's side-lane streams, see above) */
int fpd_plan_run(fpd_plan* p, int32_t begin, int32_t end, fpd_stream_t stream);
/* Issue the single op `op` on `stream` itself, ignoring its lane and waits (measurement aid: bench.py re-launches one
 * recorded op back to back between two events to time a kernel exactly as the step launches it). */
int fpd_plan_run_op(fpd_plan* p, int32_t op, fpd_stream_t stream);
/* capture ops [begin,end) into a hipGraph once, then replay it (graph id returned by capture) */
int fpd_plan_capture(fpd_plan* p, int32_t begin, int32_t end, fpd_stream_t stream);
int fpd_plan_replay(fpd_plan* p, int32_t graph_id, fpd_stream_t stream);

/* ---- misc ---- */
const char* fpd_last_error(void);
int fpd_set_backend(int32_t backend);         /* FPD_BACKEND_*; returns previous */
/* run-time knobs (process-wide; the defaults are what the product uses): "conv_pp" = 0 never / 1 launches with >= 256 pixel
 * tiles (default) / 2 whenever in its domain: use of the persistent convolution kernel for big maps (csrc/conv_pp.hip);
 * "conv_pp_blocks" = its persistent blocks per occupancy slot (default 256); "bneck_blocks" / "head_blocks" = grid caps of the
 * persistent fpd_bottleneck_forward / fpd_head_forward kernels (defaults 128 / 160, any n >= 1); "wgrad_tile_only" = 1: fpd_conv_wgrad() fails
 * instead of falling through to the generic kernels when the halo-tile kernel declines a shape (tests); "conv_skip" / "stem_act" =
 * 0: fpd_conv_skip_supported() / fpd_stem_act_supported() answer 0 and such launches are refused (default 1); "bneck_upadd" = 0: fpd_bneck_upadd_supported() answers 0 and a Bottleneck
 * launch with x2 is refused (default 1, or what FPD_BNECK_UPADD says); "ew_merge" = 0:
 * the same for fpd_ew_merge_supported() / fpd_ew_merge() (default 1, or what FPD_EW_MERGE says); "ew_merge_blocks" = grid cap of those launches (default 2048, any
 * n >= 1); "ew_blocks" = n >= 1: no fpd_elementwise() launch, neither half of an fpd_elementwise_pair() launch and no fpd_affsum() launch
 * gets more than n blocks, so that a thread walks several pixels on a small tensor (tests); 0 = the library's own grid rule alone
 * (default); a negative value changes nothing; "stem_blocks" = n >= 1: no persistent stem launch -- the space-to-depth forward
 * and the three weight gradients of fpd_stem_wgrad() -- gets more than n blocks, and fpd_stem_wgrad_num_partials() answers
 * accordingly, so that a block owns several tiles on a small image (tests); 0 = the kernels' own grids alone (default), a negative
 * value changes nothing; a launch without slabs (partial == NULL) keeps its single block; "stem_s2d_launches" /
 * "stem_mfma_launches" = read-only (the value is ignored): fpd_stem_forward() + fpd_stem_wgrad() launches served so far by the
 * space-to-depth kernels (csrc/stem_s2d.hip) / the im2col kernels (csrc/stem_mfma.hip); a stem launch that moves neither was
 * served by the direct kernels (csrc/stem.hip); "conv_c1_launches" / "conv_c3_launches" / "conv_tile_launches" = read-only:
 * convolution launches served so far by csrc/conv_c1.hip / conv_c3.hip / conv_tile.hip; "wgrad_tile_launches" = read-only:
 * launches of wgrad_tile_kernel itself (csrc/wgrad_tile.hip; those its launch function hands to wgrad3 are not counted);
 * "wgrad3_launches" = read-only: the fpd_conv_wgrad() launches served by csrc/wgrad3.hip.  Returns the
 * previous value (>= 0; 0 for "wgrad_tile_only"), negative = unknown option. */
int fpd_set_option(const char* name, int32_t value);
int fpd_abi_sizeof(const char* struct_name);  /* sizeof of a struct above, -1 if unknown */
/* Version of everything sizeof cannot see (buffer encodings and sizes).  History: 1 = statistics as fp64 [R][2][C] (rounds 1-3)
 * and, mistakenly unchanged, the first integer-limb encoding of round 4; 2 = fpd_stat_t limbs [R][2][2][C] with hi in units of
 * 2^-20 (twice the bytes of version 1's buffers: a host built against version 1 must not run).  Hosts assert
 * fpd_abi_version() == FPD_ABI_VERSION and size statistics buffers with fpd_stats_words(). */
#define FPD_ABI_VERSION 2
int fpd_abi_version(void);
int64_t fpd_stats_words(int32_t channels);    /* 64-bit words of one statistics buffer over `channels` = FPD_STATS_WORDS(channels) */
/* in-stream timing helpers (HIP events on `stream`): returns elapsed ms of [start,stop) */
void* fpd_event_create(void);
int fpd_event_record(void* ev, fpd_stream_t stream);
float fpd_event_elapsed_ms(void* start, void* stop); /* synchronises on stop */
void fpd_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* FPD_AMD_H */
