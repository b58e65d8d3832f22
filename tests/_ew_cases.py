"""Case tables of tests/test_elementwise_gpu.py (the plain elementwise kernels of csrc/elementwise.hip: ew_kernel,
ew_pair_kernel, affsum_kernel) and the host-side grid rule they are launched with, restated in plain Python so that
tests/test_ew_cases_cpu.py can say -- without a GPU -- which launches make several trips of the pixel loop.

Grid rule (csrc/elementwise.hip ew_rule / fpd_affsum_launch): a thread owns one 16-byte channel vector (VEC = 4 fp32 / 8 bf16
elements), VP = C / VEC vectors make a pixel, a block of 256 threads steps over PB = 256 / VP pixels at a time, and
grid = min(cdiv(npix, PB), cap) with cap = 512 for launches that end in statistics atomics and 2048 otherwise; option
"ew_blocks" = n >= 1 puts min(., n) on top.  npix is the iteration space: N*H*W, or N*(H/2)*(W/2) for the pooled ops."""

# (N, H, W, C)
MULTI = (3, 12, 10, 64)         # the multi-trip shape: 360 full-resolution / 90 pooled pixels, no multiple of any blocks * PB
SHAPES = [
    MULTI,
    (2, 4, 4, 8),               # C = 8: in bf16 one vector per pixel (VP = 1, PB = 256)
    (1, 4, 6, 48),              # 256 % VP != 0: idle threads behind the `active` guard
    (1, 4, 4, 384),             # HRNet-W48's widest branch: PB = 5 (bf16) / 2 (fp32)
    (1, 2, 4, 512),             # FPD_MAXC: VP = 128 in fp32 (the host check's limit), full LDS tables
]
INPLACE_SHAPES = [MULTI, (1, 4, 6, 48)]
CAPS = (1, 3)                   # values of option "ew_blocks" of the multi-trip runs
DTYPES = (0, 1)                 # FPD_F32, FPD_BF16
VEC = {0: 4, 1: 8}

POOLED = ('maxpool_fwd', 'maxpool_bwd', 'sumpool')                  # iterate over the half-resolution tensor
STATS_OPS = ('bnrelu_fwd', 'maxpool_fwd', 'upadd_fwd')              # cap 512 when out_stats is given
EW_OPS = ('bnrelu_fwd', 'bnrelu_bwd_r', 'bn_bwd_apply', 'maxpool_fwd', 'maxpool_bwd', 'upadd_fwd', 'sumpool', 'add',
          'relu_mask', 'dilate2')


def half(shape):
    n, h, w, c = shape
    return (n, h // 2, w // 2, c)


def b1_launches(shape):
    """(label, op, dims, ends in statistics) of every launch of the all-ops list (test_elementwise_gpu.Case)."""
    out = []
    for op in EW_OPS:
        out.append((op, op, shape, op in STATS_OPS or op == 'bnrelu_bwd_r'))
    out.append(('maxpool_bwd without add', 'maxpool_bwd', shape, False))
    return out


def b2_launches():
    """The launches of the multi-trip runs: all of b1_launches(MULTI), the variants (same ops, with and without statistics),
    the four-term affsum and the two halves of the bn_bwd_apply pair."""
    out = b1_launches(MULTI)
    out += [(op + ' without statistics', op, MULTI, False) for op in STATS_OPS]
    out += [('affsum', 'affsum', MULTI, False),
            ('pair, full resolution', 'bn_bwd_apply', MULTI, False),
            ('pair, half resolution', 'bn_bwd_apply', half(MULTI), False)]
    return out


def cdiv(a, b):
    return (a + b - 1) // b


def pixels_per_step(C, dtype):
    vp = C // VEC[dtype]
    assert C % VEC[dtype] == 0 and 1 <= vp <= 128
    return 256 // vp


def npix(op, dims):
    n, h, w, _ = dims
    return n * (h // 2) * (w // 2) if op in POOLED else n * h * w


def grid(op, dims, dtype, stats, ew_blocks=0, stats_blocks=512):
    g = max(1, min(cdiv(npix(op, dims), pixels_per_step(dims[3], dtype)), stats_blocks if stats else 2048))
    return min(g, ew_blocks) if ew_blocks >= 1 else g


def trips(op, dims, dtype, stats, ew_blocks=0):
    """(trips of the busiest thread, pixels of the last trip over the whole grid, pixels of a full trip)."""
    per_trip = grid(op, dims, dtype, stats, ew_blocks) * pixels_per_step(dims[3], dtype)
    n = npix(op, dims)
    t = cdiv(n, per_trip)
    return t, n - (t - 1) * per_trip, per_trip
