"""Shapes shared by tests/test_conv_skip_gpu.py and tests/test_skip_lowering_cpu.py: conv3 of a downsample Bottleneck with the
skip 1x1 as its second source (fpd_conv_t.x2).  (N, H, W, C, K, bn, stats, blocks) with C2 = C: 32-pixel tiles, rounds of 8."""

SKIP_CASES = [
    (2, 64, 64, 64, 128, 'eval', False, 5),        # teacher layer1 class, uneven round ranges
    (1, 128, 128, 32, 64, 'train', True, 7),       # student layer1, 128-wide rows
    (2, 32, 32, 64, 128, 'train', True, 3),        # student layer2
    (1, 4, 40, 64, 128, 'train', True, 2),         # 5 tiles: ragged last round
    (3, 4, 8, 32, 64, 'train', True, 1),           # 3 tiles in one round
    (2, 32, 32, 32, 64, 'eval', False, 256),       # more blocks than rounds
    (2, 32, 32, 128, 256, 'eval', False, 4),       # K = 256
    (1, 4, 40, 128, 256, 'eval', False, 3),        # K = 256
]


def served(case):
    """The streaming kernel forms the second source for C -> 2C with C in {32, 64}.  K = 256 (the teacher's layer2) is outside its
    channel domain and the two-halves launch for it is not built: those launches stay two conv_tile launches."""
    return case[3] in (32, 64) and case[4] == 2 * case[3]
