"""The numpy restatement of the DARK decode (include/fpd_amd.h, fpd_dark_t) and the cases the DARK tests share.

`decode(maps, k, dtype)` restates the specification for [N,J,H,W] maps with taps, blur, rescaling and logarithm in `dtype`;
the 13-value Newton step is float64 either way (`newton`).  The float64 restatement is the yardstick, the float32 one
supplies the error scale E32 of a kernel that stores its blurred images as float32.  `blur_published` is the padded form
of the published code (zero padding of (k-1)/2, then a blur with a reflecting border that is never reached).

Unpinned: neither cv2.GaussianBlur nor the DarkPose source is available to these tests, so everything here equals the
written specification, not a run of the authors' code."""
import numpy as np

# (N, J, H, W, k) of the GPU tests
SHAPES = {'S1': (2, 3, 16, 12, 11), 'S2': (2, 5, 20, 28, 9), 'S3': (1, 17, 64, 48, 11), 'S4': (2, 3, 10, 8, 11),
          'S5': (1, 2, 128, 128, 11)}
MIN_DET = 1e-3


def taps(k, dtype=np.float64):
    """OpenCV's getGaussianKernel(k, 0) for k > 7, computed in float64 and rounded to dtype."""
    assert k % 2 == 1 and 9 <= k <= 31
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    t = np.exp(-0.5 / (sigma * sigma) * (np.arange(k, dtype=np.float64) - (k - 1) / 2) ** 2)
    return (t / t.sum()).astype(dtype)


def _conv_zero(m, t, axis):
    """out[i] = sum_d t[d] * m[i + d - r] along `axis`, zeros outside, taps in ascending order, every product and sum in m.dtype."""
    k, r, n = len(t), len(t) // 2, m.shape[axis]
    out = np.zeros_like(m)
    src = [slice(None)] * m.ndim
    dst = [slice(None)] * m.ndim
    for d in range(k):
        lo, hi = max(0, r - d), min(n, n + r - d)              # output positions whose tap d lies inside the map
        if lo >= hi:
            continue
        dst[axis], src[axis] = slice(lo, hi), slice(lo + d - r, hi + d - r)
        out[tuple(dst)] += t[d] * m[tuple(src)]
    return out


def blur(m, k, dtype=np.float64):
    """Rows first, then columns, zeros outside the map.  m: [..., H, W]."""
    t = taps(k, dtype)
    m = m.astype(dtype)
    return _conv_zero(_conv_zero(m, t, m.ndim - 1), t, m.ndim - 2)


def blur_published(m, k):
    """The published form in float64 for one [H, W] map: pad with (k-1)/2 zeros, blur with a reflecting (BORDER_REFLECT_101)
    border, cut the middle out again."""
    r = (k - 1) // 2
    t = taps(k)
    h, w = m.shape
    dr = np.zeros((h + 2 * r, w + 2 * r))
    dr[r:h + r, r:w + r] = m

    def reflect101(a, axis):
        n = a.shape[axis]
        idx = np.arange(-r, n + r)
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
        return np.take(a, idx, axis=axis)

    def conv(a, axis):
        n = a.shape[axis]
        ext = reflect101(a, axis)
        out = np.zeros_like(a)
        for d in range(k):
            out += t[d] * np.take(ext, np.arange(d, d + n), axis=axis)
        return out

    return conv(conv(dr, 1), 0)[r:h + r, r:w + r]


def gather13(L, px, py):
    """The 13 values of L around (px, py) in the order of csrc/dark_math.h."""
    ox = (0, 1, -1, 0, 0, 2, -2, 0, 0, 1, 1, -1, -1)
    oy = (0, 0, 0, 1, -1, 0, 0, 2, -2, 1, -1, 1, -1)
    return np.array([L[py + b, px + a] for a, b in zip(ox, oy)], dtype=np.float64)


def newton(v):
    """(refined, ox, oy, det) of the 13 float64 values v: csrc/dark_math.h's fpd_dark_step, operation for operation."""
    v = np.asarray(v, dtype=np.float64)
    dx = 0.5 * (v[1] - v[2])
    dy = 0.5 * (v[3] - v[4])
    dxx = 0.25 * (v[5] - 2.0 * v[0] + v[6])
    dyy = 0.25 * (v[7] - 2.0 * v[0] + v[8])
    dxy = 0.25 * (v[9] - v[10] - v[11] + v[12])
    det = dxx * dyy - dxy * dxy
    if not det != 0.0:
        return 0, np.float64(0.0), np.float64(0.0), det
    return 1, -(dyy * dx - dxy * dy) / det, -(dxx * dy - dxy * dx) / det, det


def argmax_coords(maps):
    """get_max_preds: (coords [N,J,2] float32, maxvals [N,J] float32, idx), first maximum wins, (0, 0) where the maximum is <= 0."""
    n, j, h, w = maps.shape
    flat = maps.reshape(n, j, -1)
    idx = flat.argmax(2)
    maxvals = np.take_along_axis(flat, idx[..., None], 2)[..., 0].astype(np.float32)
    coords = np.stack([idx % w, idx // w], -1).astype(np.float32)
    coords *= (maxvals > 0)[..., None]
    return coords, maxvals, idx


def decode(maps, k, dtype=np.float64):
    """(coords [N,J,2] float32, maxvals [N,J] float32, refined [N,J] int32, det [N,J] float64) of float32 maps [N,J,H,W]."""
    maps = np.asarray(maps, dtype=np.float32)
    n, j, h, w = maps.shape
    coords, maxvals, _ = argmax_coords(maps)
    refined = np.zeros((n, j), np.int32)
    dets = np.zeros((n, j), np.float64)
    B = blur(maps, k, dtype)
    for a in range(n):
        for b in range(j):
            mv = maxvals[a, b]
            px, py = int(coords[a, b, 0]), int(coords[a, b, 1])
            if not (mv > 0 and 1 < px < w - 2 and 1 < py < h - 2):
                continue
            bm = B[a, b].max()
            if not bm > 0:
                continue
            L = np.log(np.maximum(B[a, b] * (dtype(mv) / bm), dtype(1e-10)))
            assert L.dtype == dtype
            r, ox, oy, det = newton(gather13(L, px, py))
            refined[a, b], dets[a, b] = r, det
            if r:
                off = np.array([ox, oy], dtype=np.float64)
                coords[a, b] += off                                    # float32 += float64: one rounding of the float64 sum
    return coords, maxvals, refined, dets


def blob(h, w, mx, my, amp):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return amp * np.exp(-((x - mx) ** 2 + (y - my) ** 2) / 8.0)


def random_case(name, seed=None):
    """(maps [N,J,H,W] float32, centres [N,J,2], k) of shape `name`: blobs of sigma 2 with sub-pixel centres in
    [2.5, W-3.5] x [2.5, H-3.5], amplitude in [0.3, 1], plus N(0, 0.01) noise.  Asserts the input condition: the float64
    restatement refines every (sample, joint) with |det| >= MIN_DET, so that no discrete decision hangs on rounding."""
    n, j, h, w, k = SHAPES[name]
    rng = np.random.RandomState(sum(map(ord, name)) * 1000 + h * 131 + w if seed is None else seed)
    cen = np.stack([rng.uniform(2.5, w - 3.5, (n, j)), rng.uniform(2.5, h - 3.5, (n, j))], -1)
    amp = rng.uniform(0.3, 1.0, (n, j))
    maps = np.zeros((n, j, h, w), np.float32)
    for a in range(n):
        for b in range(j):
            maps[a, b] = (blob(h, w, cen[a, b, 0], cen[a, b, 1], amp[a, b]) + 0.01 * rng.randn(h, w)).astype(np.float32)
    _, _, refined, det = decode(maps, k)
    assert refined.all() and (np.abs(det) >= MIN_DET).all(), (name, refined, det)
    return maps, cen, k


def designed_case(h=16, w=12, k=11):
    """([1,J,H,W] float32 maps, names) of the designed maps: a narrow blob whose arg-max sits at px in {0, 1, 2, W-3, W-2,
    W-1} (py mid-map) and the same in y, a map without a positive value, a single spike on zeros, two equal maxima."""
    maps, names = [], []
    for px in (0, 1, 2, w - 3, w - 2, w - 1):
        maps.append(blob(h, w, px + 0.2 * (1 if px < w // 2 else -1), h // 2 + 0.3, 0.8))
        names.append('px=%d' % px)
    for py in (0, 1, 2, h - 3, h - 2, h - 1):
        maps.append(blob(h, w, w // 2 - 0.3, py + 0.2 * (1 if py < h // 2 else -1), 0.7))
        names.append('py=%d' % py)
    maps.append(-blob(h, w, 5.0, 6.0, 0.5) - 0.01)
    names.append('not positive')
    spike = np.zeros((h, w))
    spike[7, 5] = 0.6
    maps.append(spike)
    names.append('spike')
    twin = blob(h, w, 4.0, 5.0, 0.5) + blob(h, w, 8.0, 10.0, 0.5)              # both peaks on pixel centres, the same value
    twin[10, 8] = twin[5, 4] = max(twin[10, 8], twin[5, 4])
    maps.append(twin)
    names.append('two maxima')
    m = np.stack(maps).astype(np.float32)[None]
    # the designed arg-max positions are what they are meant to be
    c, v, _ = argmax_coords(m)
    for q, px in enumerate((0, 1, 2, w - 3, w - 2, w - 1)):
        assert c[0, q, 0] == px and c[0, q, 1] == h // 2, (q, c[0, q])
    for q, py in enumerate((0, 1, 2, h - 3, h - 2, h - 1)):
        assert c[0, 6 + q, 1] == py and c[0, 6 + q, 0] == w // 2, (q, c[0, 6 + q])
    assert v[0, 12] <= 0 and tuple(c[0, 12]) == (0, 0)
    assert tuple(c[0, 13]) == (5, 7) and tuple(c[0, 14]) == (4, 5) and m[0, 14, 10, 8] == m[0, 14, 5, 4]
    return m, names


def designed_expectation(names, w=12, h=16):
    """What the guards say about the designed maps, independent of the decode."""
    want = []
    for nm in names:
        if nm.startswith('px='):
            want.append(int(1 < int(nm[3:]) < w - 2))
        elif nm.startswith('py='):
            want.append(int(1 < int(nm[3:]) < h - 2))
        elif nm == 'not positive':
            want.append(0)
        else:
            want.append(1)
    return np.array(want, np.int32)
