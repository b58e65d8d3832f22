"""numpy restatement of csrc/ema_math.h (the weight average of utils.ModelEma / fpd_ema), in its operation order:
    u = updates_done + 1;  d = warmup ? min(decay, (1 + u) / (10 + u)) : decay   (float64)
    w = float32(1 - d);    e' = e + w * (x - e)                                   (three float32 roundings, never fused)
numpy rounds every float32 operation on its own, which is exactly "contraction off"."""
import numpy as np

# the ramp (1 + u) / (10 + u) reaches 0.9998 at u = 44 990, i.e. after 44 989 updates: both sides of that are in, next to the
# counts around 49 990
UPDATES = (0, 1, 8, 9, 10, 1000, 44979, 44988, 44989, 44990, 44999, 49989, 49990, 49991, 10 ** 7)
DECAYS = (0.0, 0.5, 0.999, 0.9998)


def weight(updates_done, decay, warmup):
    u = np.float64(int(updates_done) + 1)
    d = np.float64(decay)
    if warmup:
        ramp = (np.float64(1.0) + u) / (np.float64(10.0) + u)
        if ramp < d:
            d = ramp
    return np.float32(np.float64(1.0) - d)


def update(e, x, w):
    e, x, w = np.asarray(e, np.float32), np.asarray(x, np.float32), np.float32(w)
    with np.errstate(all='ignore'):
        diff = (x - e).astype(np.float32)
        step = (w * diff).astype(np.float32)
        return (e + step).astype(np.float32)


def update_fused(e, x, w):
    """What a contracted build would compute: fma(w, x - e, e), one rounding for the product and the sum (exact in float64:
    a float32 product has 48 significant bits, and the sum is rounded once into float32 below -- double rounding cannot
    bite on the designed triple, whose float64 sum is exact)."""
    e, x, w = np.asarray(e, np.float32), np.asarray(x, np.float32), np.float32(w)
    diff = (x - e).astype(np.float32)
    return (e.astype(np.float64) + w.astype(np.float64) * diff.astype(np.float64)).astype(np.float32)


# (e, x, w) on which the two forms differ in the last bit: x - e = 0x1.92f96p-2 is exact, w * (x - e) needs 36 bits; rounded
# to float32 first it lands on a tie of the sum's coarser grid, which then rounds to even (up): 0x1.39c344p+0, where the
# single rounding of fma gives 0x1.39c342p+0.  e = 1 and both factors below 1 keep the float64 sum of update_fused exact.
DESIGNED = (np.float32(1.0), np.float32(float.fromhex('0x1.64be58p+0')), np.float32(float.fromhex('0x1.259p-1')))
DESIGNED_UNFUSED, DESIGNED_FUSED = np.float32(float.fromhex('0x1.39c344p+0')), np.float32(float.fromhex('0x1.39c342p+0'))


def special_values():
    """(e, x) pairs over denormals, +-0, +-inf and NaN, every one against every other."""
    tiny = np.float32(1e-45)
    v = np.array([0.0, -0.0, tiny, -tiny, np.float32(1.1754942e-38), 1.0, -1.0, 3.4028235e38, -3.4028235e38, np.inf, -np.inf,
                  np.nan], np.float32)
    e, x = np.meshgrid(v, v, indexing='ij')
    return e.reshape(-1).copy(), x.reshape(-1).copy()


def seeded(n, seed=0):
    rng = np.random.RandomState(seed)
    e = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
    x = (e + rng.standard_normal(n).astype(np.float32) * np.abs(e) * np.float32(0.01)).astype(np.float32)
    return e, x


def run(e_list, x_lists, copy_lists, decay, warmup, updates_done=0):
    """Successive updates of several segments: e_list[s] float32 arrays (updated copies are returned), x_lists[k][s] the
    source of update k; the copied integers are those of the last update."""
    e_list = [np.array(e, np.float32) for e in e_list]
    for k, xs in enumerate(x_lists):
        w = weight(updates_done + k, decay, warmup)
        e_list = [update(e, x, w) for e, x in zip(e_list, xs)]
    return e_list, updates_done + len(x_lists)
