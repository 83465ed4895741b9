"""Mutants of the restatement of the speckle contract (tests/fe_speckle_ref.py): each one restates the labelling with one
plausible device error in it -- the errors a tiled union-find can make: diagonal neighbours, an off-by-one in either
comparison, the difference against the wrong pixel or in the wrong type, unions lost where two tiles meet.
tests/test_fe_speckle_cpu.py holds that the planes made on purpose tell every one of them from the restatement, and
names the plane: a kernel with that error would fail the byte comparison of tests/test_gpu_fe_speckle.py.  Python
only; nothing here ever runs against the GPU."""
import numpy as np

import fe_speckle_ref as K


def _pairs(q, max_diff, diagonals=False, strict=False, wrap=False):
    """K.joined_pairs with one error: the two upper diagonal neighbours joined too; `<` for `<=`; the difference of
    uint16 values that wraps (and the smaller way round taken)"""
    q = np.asarray(q)
    h, w = q.shape
    v = q.astype(np.int64)
    idx = np.arange(h * w).reshape(h, w)

    def near(a, b):
        d = np.abs(a - b)
        if wrap:
            d = np.minimum((a - b) & 0xFFFF, (b - a) & 0xFFFF)
        return (a != 0) & (b != 0) & ((d < max_diff) if strict else (d <= max_diff))

    views = [((slice(None), slice(1, None)), (slice(None), slice(None, -1))),
             ((slice(1, None), slice(None)), (slice(None, -1), slice(None)))]
    if diagonals:
        views += [((slice(1, None), slice(1, None)), (slice(None, -1), slice(None, -1))),
                  ((slice(1, None), slice(None, -1)), (slice(None, -1), slice(1, None)))]
    a, b = [], []
    for s, t in views:
        m = near(v[s], v[t])
        a.append(idx[s][m])
        b.append(idx[t][m])
    return np.concatenate(a), np.concatenate(b)


def eight_connected(q, sp):
    return K.filter_plane(q, sp, K.sizes_of_pairs(q, *_pairs(q, sp[1], diagonals=True)))


def size_strict(q, sp):
    """`<` in place of `<=` on the size"""
    sizes = K.components(q, sp[1])
    gone = (np.asarray(q) != 0) & (sizes < sp[0])
    return np.where(gone, 0, q).astype(np.uint16), sizes, int(np.count_nonzero(gone))


def diff_strict(q, sp):
    """`<` in place of `<=` on the difference"""
    return K.filter_plane(q, sp, K.sizes_of_pairs(q, *_pairs(q, sp[1], strict=True)))


def against_first_pixel(q, sp):
    """the difference taken against the component's first pixel in scan order, not against the neighbour"""
    return K.filter_plane(q, sp, K.flood(q, sp[1], against_first=True))


def uint16_wrap(q, sp):
    return K.filter_plane(q, sp, K.sizes_of_pairs(q, *_pairs(q, sp[1], wrap=True)))


def seam_cut(q, sp, period, vertical_border):
    """unions lost across every border `period` pixels apart: between columns k * period - 1 and k * period
    (`vertical_border`), or between such rows"""
    w = np.asarray(q).shape[1]
    a, b = K.joined_pairs(q, sp[1])
    if vertical_border:
        lost = (a - b == 1) & ((a % w) % period == 0)
    else:
        lost = (a - b == w) & ((a // w) % period == 0)
    return K.filter_plane(q, sp, K.sizes_of_pairs(q, a[~lost], b[~lost]))


SEAMS = [(period, vertical) for period in (16, 32, 64) for vertical in (True, False)]
