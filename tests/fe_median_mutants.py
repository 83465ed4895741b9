"""Mutants of the restatement of the median contract (tests/fe_median_ref.py): each one restates the stage with one
plausible device error in it -- the errors a tiled median of a variable number of values can make: the wrong middle, a
zero or a pixel outside the image taken for a value, a result read back as a neighbour's input, a 16-bit sentinel that
is also a depth, an off-by-one in the fill test or in the window, neighbours lost where two tiles meet.
tests/test_fe_median_cpu.py holds that the planes made on purpose tell every one of them from the restatement, and
names the plane and the settings: a kernel with that error would fail the byte comparison of
tests/test_gpu_fe_median.py.  Python only; nothing here ever runs against the GPU."""
import numpy as np

import fe_median_ref as K

BIG = 1 << 20


def _pick(W, member, A, m, index=None, strict_fill=False):
    """K.median on a stack of window planes W with its members marked: `index(n)` in place of (n - 1) >> 1"""
    radius, fill_min = m
    n = member.sum(axis=0)
    keys = np.sort(np.where(member, W, BIG), axis=0)
    idx = np.maximum((n - 1) >> 1, 0) if index is None else index(n)
    med = np.take_along_axis(keys, idx[None], axis=0)[0]
    med = np.where(med == BIG, 0, med)
    enough = (n > fill_min) if strict_fill else (n >= fill_min)
    fill = (A == 0) & (fill_min > 0) & enough
    return K.finish(A, np.where((A != 0) | fill, med, 0))


def upper_median(A, m):
    """v_(n >> 1)"""
    W = K.windows(A, m[0])
    return _pick(W, W > 0, np.asarray(A), m, index=lambda n: np.minimum(n >> 1, np.maximum(n - 1, 0)))


def zeros_counted(A, m):
    """a pixel of the image without depth is a member with the value 0"""
    W = K.windows(A, m[0])
    return _pick(W, W >= 0, np.asarray(A), m)


def replicated_border(A, m):
    """a pixel outside the image is the nearest pixel of the image"""
    A = np.asarray(A)
    r = m[0]
    h, w = A.shape
    P = np.pad(A.astype(np.int64), r, mode="edge")
    W = np.stack([P[r + dy:r + dy + h, r + dx:r + dx + w] for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
    return _pick(W, W > 0, A, m)


def in_place(A, m):
    """filtered in place in scan order: a pixel's window holds the results of the pixels before it"""
    A = np.asarray(A)
    radius, fill_min = m
    h, w = A.shape
    B = A.astype(np.int64).copy()
    for y in range(h):
        for x in range(w):
            win = B[max(y - radius, 0):y + radius + 1, max(x - radius, 0):x + radius + 1]
            V = np.sort(win[win != 0])
            n = len(V)
            if B[y, x] != 0 or (fill_min > 0 and n >= fill_min):
                B[y, x] = V[(n - 1) >> 1] if n else 0
    return K.finish(A, B)


def max_is_none(A, m):
    """65535 taken for "none": no member of a window, and a pixel that holds it a pixel without depth"""
    A = np.asarray(A)
    W = K.windows(A, m[0])
    B = _pick(W, (W > 0) & (W != 65535), np.where(A == 65535, 0, A), m)[0]
    return K.finish(A, B)


def fill_strict(A, m):
    """n > fill_min for n >= fill_min"""
    W = K.windows(A, m[0])
    return _pick(W, W > 0, np.asarray(A), m, strict_fill=True)


def fixed_middle(A, m):
    """the middle of a sort padded with "none" to the full window, whatever n is (a "none" picked is no depth)"""
    W = K.windows(A, m[0])
    return _pick(W, W > 0, np.asarray(A), m, index=lambda n: np.full(n.shape, W.shape[0] // 2))


def short_window(A, m):
    """the window one pixel short in x: dx = -r .. r - 1"""
    W = K.windows(A, m[0])
    side = 2 * m[0] + 1
    keep = np.array([k % side != side - 1 for k in range(side * side)])
    return _pick(W, (W > 0) & keep[:, None, None], np.asarray(A), m)


def tile_cut(A, m, tw, th):
    """neighbours outside the pixel's own tile of tw x th pixels dropped: no halo"""
    A = np.asarray(A)
    r = m[0]
    h, w = A.shape
    W = K.windows(A, r)
    ty, tx = (np.arange(h) // th)[:, None], (np.arange(w) // tw)[None, :]
    same = []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            yy, xx = np.arange(h)[:, None] + dy, np.arange(w)[None, :] + dx
            same.append((yy // th == ty) & (xx // tw == tx))
    return _pick(W, (W > 0) & np.stack(same), A, m)


TILES = [(32, 8), (64, 4), (16, 16), K.TILE]
PLAIN = [upper_median, zeros_counted, replicated_border, in_place, max_is_none, fill_strict, fixed_middle, short_window]
