"""The unpack contract of include/cvo_frontend.h (at CVO_FE_PIXEL_*) restated in numpy: the layout table, the byte
moves, BT.601 limited range in int32 with an arithmetic shift, and the bilinear demosaic with a mirrored border.  The
building blocks (yuv_planes, bt601, padded, demosaic) are what tests/fe_unpack_mutants.py recombines wrongly.

Behind them the test side: packers (a mosaic, a forward BT.601 with subsampled chroma -- part of no contract, they
only make plausible inputs) and the list of inputs the GPU test runs, which tests/test_fe_unpack_cpu.py holds against
the mutants."""
import numpy as np

(BGR8, RGB8, BGRA8, RGBA8, GREY8, YUY2, UYVY, NV12, BAYER_RGGB8, BAYER_BGGR8, BAYER_GRBG8, BAYER_GBRG8) = range(12)
FORMATS = tuple(range(12))
NAMES = ("BGR8", "RGB8", "BGRA8", "RGBA8", "GREY8", "YUY2", "UYVY", "NV12", "BAYER_RGGB8", "BAYER_BGGR8", "BAYER_GRBG8",
         "BAYER_GBRG8")
YUV = (YUY2, UYVY, NV12)
BAYER = (BAYER_RGGB8, BAYER_BGGR8, BAYER_GRBG8, BAYER_GBRG8)
BYTES_PER_PIXEL = {BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4, GREY8: 1, YUY2: 2, UYVY: 2, NV12: 1, BAYER_RGGB8: 1,
                   BAYER_BGGR8: 1, BAYER_GRBG8: 1, BAYER_GBRG8: 1}
# the parities (x, y) of the mosaic's red pixel: the four letters are pixels (0,0) (1,0) / (0,1) (1,1)
RED = {BAYER_RGGB8: (0, 0), BAYER_BGGR8: (1, 1), BAYER_GRBG8: (1, 0), BAYER_GBRG8: (0, 1)}


def fits(fmt, w, h):
    if fmt not in FORMATS or w < 1 or h < 1:
        return False
    if fmt in YUV and w % 2:
        return False
    if fmt == NV12 and h % 2:
        return False
    return not (fmt in BAYER and (w < 2 or h < 2))


def layout(fmt, w, h):
    """(rows, row_bytes) of a packed w x h image, or None for a format the size does not fit"""
    if not fits(fmt, w, h):
        return None
    return (h + h // 2 if fmt == NV12 else h), w * BYTES_PER_PIXEL[fmt]


# ---- YUV ---------------------------------------------------------------------------------------------

def yuv_planes(src, fmt, w, h):
    """Y, U, V of every pixel (int32, h x w): pixels 2k and 2k+1 share their pair's chroma, NV12 row y takes chroma
    row y >> 1; nothing is interpolated"""
    s = np.asarray(src, np.uint8).reshape(layout(fmt, w, h)).astype(np.int32)
    if fmt == NV12:
        uv = s[h:].reshape(h // 2, w // 2, 2)
        rows = np.arange(h) >> 1
        return s[:h], np.repeat(uv[rows, :, 0], 2, axis=1), np.repeat(uv[rows, :, 1], 2, axis=1)
    q = s.reshape(h, w // 2, 4)
    if fmt == YUY2:
        y, u, v = q[:, :, (0, 2)], q[:, :, 1], q[:, :, 3]
    else:
        y, u, v = q[:, :, (1, 3)], q[:, :, 0], q[:, :, 2]
    return y.reshape(h, w), np.repeat(u, 2, axis=1), np.repeat(v, 2, axis=1)


def accumulators(Y, U, V):
    """the three sums in front of the shift, in Python's wide integers' stand-in int64 (so that the int32 bound can be
    asserted rather than assumed): R, G, B"""
    c, d, e = Y.astype(np.int64) - 16, U.astype(np.int64) - 128, V.astype(np.int64) - 128
    return (1220945 * c + 1673555 * e + 524288, 1220945 * c - 410793 * d - 852458 * e + 524288,
            1220945 * c + 2115221 * d + 524288)


def bt601(Y, U, V):
    """B G R (uint8, ... x 3): >> on a signed numpy integer is the arithmetic shift of the contract"""
    r, g, b = (np.clip(a >> 20, 0, 255) for a in accumulators(Y, U, V))
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


# ---- Bayer -------------------------------------------------------------------------------------------

def padded(m):
    """the mosaic with its one-pixel border, mirrored about the border pixel (-1 -> 1, w -> w - 2): int32 (h+2) x (w+2)"""
    return np.pad(np.asarray(m, np.int32), 1, mode="reflect")


def demosaic(P, red):
    """bilinear, from the padded mosaic P: B G R (uint8, h x w x 3)"""
    h, w = P.shape[0] - 2, P.shape[1] - 2
    own = P[1:h + 1, 1:w + 1]
    n, s, wst, est = P[0:h, 1:w + 1], P[2:h + 2, 1:w + 1], P[1:h + 1, 0:w], P[1:h + 1, 2:w + 2]
    cross = (n + s + est + wst + 2) >> 2
    diag = (P[0:h, 0:w] + P[0:h, 2:w + 2] + P[2:h + 2, 0:w] + P[2:h + 2, 2:w + 2] + 2) >> 2
    horiz, vert = (est + wst + 1) >> 1, (n + s + 1) >> 1
    return assemble(own, cross, diag, horiz, vert, red)


def assemble(own, cross, diag, horiz, vert, red):
    h, w = own.shape
    px = ((np.arange(w) & 1) ^ red[0])[None, :] + np.zeros((h, 1), np.int64)
    py = ((np.arange(h) & 1) ^ red[1])[:, None] + np.zeros((1, w), np.int64)
    green, blue_row = px != py, py == 1
    of_row, other = np.where(green, horiz, own), np.where(green, vert, diag)
    g = np.where(green, own, cross)
    r, b = np.where(blue_row, other, of_row), np.where(blue_row, of_row, other)
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


# ---- the contract ------------------------------------------------------------------------------------

def unpack(src, fmt, w, h):
    """the unpacked image, h x w x 3 uint8 (B G R), of the packed bytes `src` (any shape, rows x row_bytes in C order)"""
    s = np.asarray(src, np.uint8).reshape(layout(fmt, w, h))
    if fmt == BGR8:
        return s.reshape(h, w, 3).copy()
    if fmt == RGB8:
        return s.reshape(h, w, 3)[:, :, ::-1].copy()
    if fmt == BGRA8:
        return s.reshape(h, w, 4)[:, :, :3].copy()
    if fmt == RGBA8:
        return s.reshape(h, w, 4)[:, :, 2::-1].copy()
    if fmt == GREY8:
        return np.repeat(s.reshape(h, w, 1), 3, axis=2)
    if fmt in YUV:
        return bt601(*yuv_planes(s, fmt, w, h))
    return demosaic(padded(s), RED[fmt])


def saturated(bgr):
    """the share of pixels with a channel at 0 or 255"""
    return float(np.mean(((bgr == 0) | (bgr == 255)).any(axis=-1)))


# ---- test side: packers ------------------------------------------------------------------------------

def mosaic(bgr, fmt):
    """every pixel keeps the channel of its site"""
    h, w = bgr.shape[:2]
    rx, ry = RED[fmt]
    px, py = ((np.arange(w) & 1) ^ rx)[None, :], ((np.arange(h) & 1) ^ ry)[:, None]
    return np.where(px != py, bgr[:, :, 1], np.where(py == 0, bgr[:, :, 2], bgr[:, :, 0])).astype(np.uint8)


def forward_yuv(bgr):
    """BT.601 limited range, rounded: Y, U, V per pixel (float arithmetic; only plausible, not a contract)"""
    b, g, r = (bgr[:, :, k].astype(np.float64) for k in range(3))
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    return y, u, v


def pack_yuv_planes(y, u, v, fmt):
    """full-resolution planes to the packed image: chroma is the mean of the pair (NV12: of the 2 x 2 block)"""
    h, w = y.shape
    to8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    if fmt == NV12:
        out = np.empty((h + h // 2, w), np.uint8)
        out[:h] = to8(y)
        out[h:, 0::2] = to8(u.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3)))
        out[h:, 1::2] = to8(v.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3)))
        return out
    out = np.empty((h, w // 2, 4), np.uint8)
    um, vm = to8(u.reshape(h, w // 2, 2).mean(axis=2)), to8(v.reshape(h, w // 2, 2).mean(axis=2))
    y8 = to8(y).reshape(h, w // 2, 2)
    if fmt == YUY2:
        out[:, :, 0], out[:, :, 1], out[:, :, 2], out[:, :, 3] = y8[:, :, 0], um, y8[:, :, 1], vm
    else:
        out[:, :, 0], out[:, :, 1], out[:, :, 2], out[:, :, 3] = um, y8[:, :, 0], vm, y8[:, :, 1]
    return out.reshape(h, 2 * w)


def pack(bgr, fmt, alpha=0x5A):
    """a B G R picture as a sensor of format `fmt` would deliver it: rows x row_bytes uint8"""
    bgr = np.asarray(bgr, np.uint8)
    h, w = bgr.shape[:2]
    assert fits(fmt, w, h)
    if fmt == BGR8:
        return bgr.reshape(h, w * 3).copy()
    if fmt == RGB8:
        return bgr[:, :, ::-1].reshape(h, w * 3).copy()
    if fmt in (BGRA8, RGBA8):
        out = np.full((h, w, 4), alpha, np.uint8)
        out[:, :, :3] = bgr if fmt == BGRA8 else bgr[:, :, ::-1]
        return out.reshape(h, w * 4)
    if fmt == GREY8:
        return np.clip(np.rint(forward_yuv(bgr)[0]), 0, 255).astype(np.uint8)
    if fmt in YUV:
        return pack_yuv_planes(*forward_yuv(bgr), fmt)
    return mosaic(bgr, fmt)


# ---- test side: the inputs of the GPU test ------------------------------------------------------------

SIZES = ((1, 1), (2, 1), (2, 2), (4, 2), (6, 4), (10, 6), (13, 7), (66, 18), (130, 34), (64, 64), (8192, 2), (2, 8192))
KINDS = ("random", "moderate", "zeros", "ones")
# single 255s on a mosaic of zeros: the four phases beside a corner, and beside the seam of the 64 x 16 tiles
IMPULSES = {"corner": ((0, 0), (1, 0), (0, 1), (1, 1)), "seam": ((63, 15), (64, 15), (63, 16), (64, 16))}


def sizes_for(fmt):
    """the sizes the format takes: its smallest legal one is among them (1x1, 2x1 or 2x2)"""
    return tuple(s for s in SIZES if fits(fmt, *s))


def kinds_for(fmt, w, h):
    kinds = list(KINDS)
    if fmt in BAYER and w * h <= 130 * 34:
        for where, sites in IMPULSES.items():
            kinds += ["%s-%d" % (where, k) for k, (x, y) in enumerate(sites) if x < w and y < h]
    return tuple(kinds)


def _shared(c, fmt):
    """a chroma plane constant over each pair (NV12: each 2 x 2 block), so that the packers' mean keeps its values"""
    c = np.repeat(c[:, 0::2], 2, axis=1)
    return np.repeat(c[0::2], 2, axis=0) if fmt == NV12 else c


def make_input(fmt, w, h, kind):
    """the packed image of one case, rows x row_bytes uint8; the same bytes on every call"""
    rows, row = layout(fmt, w, h)
    rng = np.random.default_rng([fmt, w, h, KINDS.index(kind) if kind in KINDS else 9])
    if kind == "zeros":
        return np.zeros((rows, row), np.uint8)
    if kind == "ones":
        return np.full((rows, row), 255, np.uint8)
    if kind == "random":
        return rng.integers(0, 256, (rows, row), dtype=np.uint8)
    if kind == "moderate":
        if fmt in YUV:   # Y in [48, 208], U and V in [96, 160]: few pixels saturate, so the arithmetic itself shows
            y = rng.integers(48, 209, (h, w)).astype(np.float64)
            u, v = (_shared(rng.integers(96, 161, (h, w)), fmt).astype(np.float64) for _ in range(2))
            return pack_yuv_planes(y, u, v, fmt)
        return pack(rng.integers(48, 209, (h, w, 3), dtype=np.uint8), fmt)
    where, k = kind.split("-")
    x, y = IMPULSES[where][int(k)]
    out = np.zeros((rows, row), np.uint8)
    out[y, x] = 255
    return out


def cases(fmt):
    """every (w, h, kind) the GPU test runs for the format"""
    return [(w, h, kind) for w, h in sizes_for(fmt) for kind in kinds_for(fmt, w, h)]
