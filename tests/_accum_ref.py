"""The numpy float32 restatement of gradient accumulation (include/fpd_amd.h, fpd_grad_accum_t; csrc/grad_accum_math.h): the
three modes of the op and a whole window of m micro-batch gradients, and the value sets the accumulation tests share.

Denormals: every value set here is chosen so that no operand and no result is subnormal.  Whether the device flushes them is
not part of the op's contract, so no test depends on it."""
import numpy as np

FIRST, ADD, FIN = 0, 1, 2
TINY = np.finfo(np.float32).tiny            # the smallest normal float32


def first(grad):
    """acc = grad, as bits."""
    return np.asarray(grad, np.float32).copy()


def add(acc, grad):
    """acc = acc + grad: one float32 addition."""
    with np.errstate(all='ignore'):
        return (np.asarray(acc, np.float32) + np.asarray(grad, np.float32)).astype(np.float32)


def scale_of(m):
    """The float32 a window of m micro-batches is multiplied by."""
    return np.float32(1.0 / m)


def fin(acc, s):
    """grad = acc * s: one float32 multiplication."""
    with np.errstate(all='ignore'):
        return (np.asarray(acc, np.float32) * np.float32(s)).astype(np.float32)


def window(grads):
    """The gradient arena behind a window of len(grads) micro-batches: acc = g0; acc = float32(acc + g_i); acc * float32(1/m)."""
    acc = first(grads[0])
    for g in grads[1:]:
        acc = add(acc, g)
    return fin(acc, scale_of(len(grads)))


def no_subnormal(*arrays):
    """True when no element of the arrays is a non-zero subnormal."""
    for a in arrays:
        a = np.asarray(a, np.float32)
        f = np.isfinite(a) & (a != 0)
        if (np.abs(a[f]) < TINY).any():
            return False
    return True


def dyadic(n, seed=0):
    """n multiples of 2^-10 in [-8, 8): sums of up to 1024 of them and their products with a power of two are exact."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-8192, 8192, size=n).astype(np.float32) / np.float32(1024.0)).astype(np.float32)


def normals(n, seed=0):
    """n standard normals, none closer to zero than 2^-20, so that sums and quotients by up to 1024 of them stay normal
    (a difference of two float32 that are at least 2^-20 in size is a multiple of 2^-44, far above the subnormal range)."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal(n).astype(np.float32)
    small = np.abs(x) < np.float32(2.0 ** -20)
    x[small] = np.float32(0.5)
    return x


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.0e38, -3.0e38, 2.0 ** -100, 1.5], np.float32)


def special_pairs():
    """(a, b): every ordered pair of SPECIALS -- covers 0 + -0, inf - inf, inf * 0 (with s = 0 excluded: s is 1/m), overflow."""
    a, b = np.meshgrid(SPECIALS, SPECIALS, indexing='ij')
    return a.ravel().copy(), b.ravel().copy()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def same(got, want):
    """Bit equality, a NaN matching any NaN (its payload is not compared)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])
