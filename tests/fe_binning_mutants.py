"""Wrong versions of the input bin (the binning contract of include/cvo_frontend.h), each the restatement
tests/fe_binning_ref.py with one mistake a kernel of this shape -- four working pixels per thread, whole dwords per
input row, keys sorted in registers -- could make.  tests/test_fe_binning_cpu.py shows for each an input of
fe_binning_ref.cases() that tells it from the restatement: the inputs the GPU test runs would show that mistake."""
import numpy as np

import fe_binning_ref as B


# ---- colour: (bgr, f) -> image -------------------------------------------------------------------------

def colour_truncates(bgr, f):
    """S / n without + (n >> 1)"""
    n = f * f
    return (B.blocks(bgr, f).astype(np.int64).sum(axis=2) // n).astype(np.uint8)


def colour_half_to_even(bgr, f):
    n = f * f
    s = B.blocks(bgr, f).astype(np.int64).sum(axis=2)
    q, r = s // n, s % n
    up = (2 * r > n) | ((2 * r == n) & (q & 1 == 1))
    return (q + up).astype(np.uint8)


def _shifted(plane, dx, dy):
    """the plane read one pixel to the side (the border replicated)"""
    fh, fw = plane.shape[:2]
    ys = np.clip(np.arange(fh) + dy, 0, fh - 1)
    xs = np.clip(np.arange(fw) + dx, 0, fw - 1)
    return plane[ys][:, xs]


def colour_origin_off_x(bgr, f):
    return B.bin_colour(_shifted(bgr, 1, 0), f)


def colour_origin_off_y(bgr, f):
    return B.bin_colour(_shifted(bgr, 0, 1), f)


def colour_xy_exchanged(bgr, f):
    """x and y exchanged where the input's size is made from the working size: the input row taken as f h pixels long
    for f w.  (With one factor for both axes nothing else can be exchanged: the members of a block are summed, in
    whatever order.)  The same image where w == h."""
    fh, fw = bgr.shape[:2]
    flat = bgr.reshape(-1, 3)
    h, w = fh // f, fw // f
    out = np.zeros((h, w, 3), np.int64)
    n = f * f
    for j in range(f):
        for i in range(f):
            yy, xx = np.mgrid[0:h, 0:w]
            idx = np.minimum((f * yy + j) * fh + (f * xx + i), fh * fw - 1)   # (fh for fw)
            out += flat[idx].astype(np.int64)
    return ((out + (n >> 1)) // n).astype(np.uint8)


def colour_last_dword_of_next_group(bgr, f):
    """per input row a thread's group is 12 f bytes; its last dword is read 12 f bytes on (the next group's last)"""
    fh, fw = bgr.shape[:2]
    rows = bgr.reshape(fh, fw * 3).copy()
    g = 12 * f
    for start in range(0, fw * 3 - g, g):
        if start + 2 * g <= fw * 3:
            rows[:, start + g - 4:start + g] = bgr.reshape(fh, fw * 3)[:, start + 2 * g - 4:start + 2 * g]
    return B.bin_colour(rows.reshape(fh, fw, 3), f)


def colour_tail_left_out(bgr, f):
    """the last w % 4 pixels of a row are not written (the output starts as zeroes)"""
    out = B.bin_colour(bgr, f)
    w = out.shape[1]
    out[:, w - w % 4:] = 0
    return out


COLOUR = (colour_truncates, colour_half_to_even, colour_origin_off_x, colour_origin_off_y, colour_xy_exchanged,
          colour_last_dword_of_next_group, colour_tail_left_out)


# ---- depth: (plane, f, depth_min) -> plane -----------------------------------------------------------

def _sorted_keys(plane, f):
    b = B.blocks(plane, f).astype(np.int64)
    return b, np.sort(np.where(b == 0, B.NONE_KEY, b), axis=2), (b != 0).sum(axis=2)


def _pick(key, pick):
    return np.take_along_axis(key, pick[..., None], axis=2)[..., 0]


def depth_upper_median(plane, f, depth_min):
    """the valid key of index k >> 1"""
    b, key, k = _sorted_keys(plane, f)
    return np.where(k >= depth_min, _pick(key, np.minimum(k >> 1, np.maximum(k - 1, 0))), 0).astype(np.uint16)


def depth_median_of_all(plane, f, depth_min):
    """the median over all n cells, zeros counted as values"""
    b, _, k = _sorted_keys(plane, f)
    n = f * f
    return np.where(k >= depth_min, np.sort(b, axis=2)[..., (n - 1) >> 1], 0).astype(np.uint16)


def depth_mean(plane, f, depth_min):
    b, _, k = _sorted_keys(plane, f)
    return np.where(k >= depth_min, b.sum(axis=2) // np.maximum(k, 1), 0).astype(np.uint16)


def depth_min_exclusive(plane, f, depth_min):
    """k > depth_min for k >= depth_min"""
    want = B.bin_depth(plane, f, depth_min)
    _, _, k = _sorted_keys(plane, f)
    return np.where(k > depth_min, want, 0).astype(np.uint16)


def depth_signed_keys(plane, f, depth_min):
    """16-bit keys compared as signed: values above 32767 sort in front of the small ones"""
    b, _, k = _sorted_keys(plane, f)
    signed = np.where(b == 0, 1 << 20, np.where(b >= 32768, b - 65536, b))
    order = np.argsort(signed, axis=2, kind="stable")
    key = np.take_along_axis(b, order, axis=2)
    return np.where(k >= depth_min, _pick(key, np.maximum(k - 1, 0) >> 1), 0).astype(np.uint16)


def depth_origin_off_x(plane, f, depth_min):
    return B.bin_depth(_shifted(plane, 1, 0), f, depth_min)


def depth_origin_off_y(plane, f, depth_min):
    return B.bin_depth(_shifted(plane, 0, 1), f, depth_min)


def depth_tail_left_out(plane, f, depth_min):
    out = B.bin_depth(plane, f, depth_min)
    w = out.shape[1]
    out[:, w - w % 4:] = 0
    return out


DEPTH = (depth_upper_median, depth_median_of_all, depth_mean, depth_min_exclusive, depth_signed_keys, depth_origin_off_x,
         depth_origin_off_y, depth_tail_left_out)


# ---- a pair: (left, right, f) -> (left, right) -----------------------------------------------------------

def pair_right_from_left(left, right, f):
    """the second plane of the launch reads the first one's input"""
    return B.bin_colour(left, f), B.bin_colour(left, f)


# ---- the camera: (fx, fy, cx, cy, f) -> the four -------------------------------------------------------

def camera_cx_over_f(fx, fy, cx, cy, f):
    """cx / f for the principal point"""
    ff = np.float32(f)
    return (np.float32(fx) / ff, np.float32(fy) / ff, np.float32(cx) / ff, np.float32(cy) / ff)
