"""Wrong versions of tests/fe_unpack_ref.py, one per way a tiled, four-pixels-per-thread unpack can go wrong.  Each is
(name, the formats it applies to, a function (src, fmt, w, h) -> B G R image).  tests/test_fe_unpack_cpu.py shows
that every one differs from the restatement on an input the GPU test runs; byte equality on the device then rules all
of them out."""
import numpy as np

import fe_unpack_ref as K

TW, TH = 64, 16   # the tile of a Bayer workgroup


def _clip8(a):
    return np.clip(a, 0, 255)


def _bgr(accs, post=_clip8, shift=20):
    r, g, b = (post(a >> shift) for a in accs)
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


def neighbour_chroma(src, fmt, w, h):
    """the chroma of the pair to the right (the last pair keeps its own)"""
    y, u, v = K.yuv_planes(src, fmt, w, h)
    x = np.minimum(np.arange(w) + 2, w - 1)
    return K.bt601(y, u[:, x], v[:, x])


def uv_exchanged(src, fmt, w, h):
    y, u, v = K.yuv_planes(src, fmt, w, h)
    return K.bt601(y, v, u)


def other_byte_order(src, fmt, w, h):
    """YUY2 read as UYVY, and UYVY as YUY2"""
    return K.unpack(src, K.UYVY if fmt == K.YUY2 else K.YUY2, w, h)


def no_rounding(src, fmt, w, h):
    return _bgr([a - 524288 for a in K.accumulators(*K.yuv_planes(src, fmt, w, h))])


def wraps(src, fmt, w, h):
    return _bgr(K.accumulators(*K.yuv_planes(src, fmt, w, h)), post=lambda a: a & 255)


def y_clamped(src, fmt, w, h):
    y, u, v = K.yuv_planes(src, fmt, w, h)
    return K.bt601(np.maximum(y, 16), u, v)


def nv12_chroma_row_y(src, fmt, w, h):
    """chroma row y in place of y >> 1 (rows past the plane's end: its last)"""
    s = np.asarray(src, np.uint8).reshape(K.layout(fmt, w, h)).astype(np.int32)
    uv = s[h:].reshape(h // 2, w // 2, 2)
    rows = np.minimum(np.arange(h), h // 2 - 1)
    return K.bt601(s[:h], np.repeat(uv[rows, :, 0], 2, axis=1), np.repeat(uv[rows, :, 1], 2, axis=1))


def _mosaic(src, fmt, w, h):
    return np.asarray(src, np.uint8).reshape(h, w).astype(np.int32)


def border_replicated(src, fmt, w, h):
    return K.demosaic(np.pad(_mosaic(src, fmt, w, h), 1, mode="edge"), K.RED[fmt])


def border_zero(src, fmt, w, h):
    return K.demosaic(np.pad(_mosaic(src, fmt, w, h), 1, mode="constant"), K.RED[fmt])


def other_phase(src, fmt, w, h):
    """RGGB read as BGGR, GRBG as GBRG, and back"""
    swap = {K.BAYER_RGGB8: K.BAYER_BGGR8, K.BAYER_BGGR8: K.BAYER_RGGB8, K.BAYER_GRBG8: K.BAYER_GBRG8, K.BAYER_GBRG8: K.BAYER_GRBG8}
    return K.unpack(src, swap[fmt], w, h)


def _terms(P, cross_round=2):
    h, w = P.shape[0] - 2, P.shape[1] - 2
    own = P[1:h + 1, 1:w + 1]
    n, s, wst, est = P[0:h, 1:w + 1], P[2:h + 2, 1:w + 1], P[1:h + 1, 0:w], P[1:h + 1, 2:w + 2]
    cross = (n + s + est + wst + cross_round) >> 2
    diag = (P[0:h, 0:w] + P[0:h, 2:w + 2] + P[2:h + 2, 0:w] + P[2:h + 2, 2:w + 2] + cross_round) >> 2
    return own, cross, diag, (est + wst + 1) >> 1, (n + s + 1) >> 1


def green_axes_exchanged(src, fmt, w, h):
    """E/W and N/S exchanged at green sites"""
    own, cross, diag, horiz, vert = _terms(K.padded(_mosaic(src, fmt, w, h)))
    return K.assemble(own, cross, diag, vert, horiz, K.RED[fmt])


def no_plus_two(src, fmt, w, h):
    own, cross, diag, horiz, vert = _terms(K.padded(_mosaic(src, fmt, w, h)), cross_round=0)
    return K.assemble(own, cross, diag, horiz, vert, K.RED[fmt])


def _tiled(src, fmt, w, h, lose_column, lose_row):
    """every tile demosaiced from its own padded copy, whose halo column right of x = 63 (mod 64) or halo row below
    y = 15 (mod 16) is the tile's own edge instead of the neighbouring tile's first pixel"""
    P = K.padded(_mosaic(src, fmt, w, h))
    out = np.empty((h, w, 3), np.uint8)
    for ty in range(0, h, TH):
        for tx in range(0, w, TW):
            th, tw = min(TH, h - ty), min(TW, w - tx)
            T = P[ty:ty + th + 2, tx:tx + tw + 2].copy()
            if lose_column and tx + TW < w:
                T[:, -1] = T[:, -2]
            if lose_row and ty + TH < h:
                T[-1, :] = T[-2, :]
            red = (K.RED[fmt][0] ^ (tx & 1), K.RED[fmt][1] ^ (ty & 1))
            out[ty:ty + th, tx:tx + tw] = K.demosaic(T, red)
    return out


def halo_column_lost(src, fmt, w, h):
    return _tiled(src, fmt, w, h, True, False)


def halo_row_lost(src, fmt, w, h):
    return _tiled(src, fmt, w, h, False, True)


def alpha_as_channel(src, fmt, w, h):
    """the three bytes behind the first in place of the first three"""
    s = np.asarray(src, np.uint8).reshape(h, w, 4)
    return (s[:, :, 1:4] if fmt == K.BGRA8 else s[:, :, 3:0:-1]).copy()


def rgb_not_swapped(src, fmt, w, h):
    return np.asarray(src, np.uint8).reshape(h, w, 3).copy()


def tail_left_out(src, fmt, w, h):
    """the last w % 4 pixels of a row never written (here: 0)"""
    out = K.unpack(src, fmt, w, h)
    if w % 4:
        out[:, w - w % 4:] = 0
    return out


def tail_from_next_row(src, fmt, w, h):
    """the last w % 4 pixels of a row are those of the row below (the last row: its own)"""
    out = K.unpack(src, fmt, w, h)
    if w % 4:
        rows = np.minimum(np.arange(h) + 1, h - 1)
        out[:, w - w % 4:] = out[rows, w - w % 4:]
    return out


ALL = tuple(f for f in K.FORMATS if f != K.BGR8)
MUTANTS = (
    ("chroma of the neighbouring pair", K.YUV, neighbour_chroma),
    ("U and V exchanged", K.YUV, uv_exchanged),
    ("YUY2 read as UYVY", (K.YUY2, K.UYVY), other_byte_order),
    ("no rounding term", K.YUV, no_rounding),
    ("wrap instead of saturate", K.YUV, wraps),
    ("Y clamped to 16 before the multiply", K.YUV, y_clamped),
    ("NV12 chroma row y instead of y >> 1", (K.NV12,), nv12_chroma_row_y),
    ("Bayer border replicated", K.BAYER, border_replicated),
    ("Bayer border zero", K.BAYER, border_zero),
    ("RGGB read as BGGR", (K.BAYER_RGGB8, K.BAYER_BGGR8), other_phase),
    ("GRBG read as GBRG", (K.BAYER_GRBG8, K.BAYER_GBRG8), other_phase),
    ("E/W and N/S exchanged at green sites", K.BAYER, green_axes_exchanged),
    (">> 2 without the + 2", K.BAYER, no_plus_two),
    ("halo column from the tile's own edge", K.BAYER, halo_column_lost),
    ("halo row from the tile's own edge", K.BAYER, halo_row_lost),
    ("alpha read as a channel", (K.BGRA8, K.RGBA8), alpha_as_channel),
    ("RGB not swapped", (K.RGB8,), rgb_not_swapped),
    ("the last w % 4 pixels of a row left out", ALL, tail_left_out),
    ("the last w % 4 pixels of a row from the next row", ALL, tail_from_next_row),
)
