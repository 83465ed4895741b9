"""A numpy restatement of the front end's median contract (include/cvo_frontend.h, at cvo_fe_depth_median): integer
planes only.  median() is the vectorised form, median_loop() the contract read out pixel by pixel; the CPU test holds
the one to the other.  k_fe_median of csrc/cvo_median.hip is held to median() by bytes.

Settings here are (radius, fill_min) pairs, or None: no filter.
Also here: the planes made on purpose, the settings and the frames the tests share."""
import numpy as np

CHANGED, FILLED = 1, 2
TILE = (64, 16)     # k_fe_median's tile, width x height
# (radius, fill_min): both radii without fill; the smallest fill_min; a majority of the 3 x 3 window's neighbours; all
# eight of them; a majority of the 5 x 5 window; all twenty-four of its neighbours
SETTINGS = [(1, 0), (2, 0), (1, 1), (1, 5), (1, 8), (2, 13), (2, 24)]
FRAME_SETTINGS = [(1, 0), (2, 0), (1, 5), (2, 13)]
LONG_SETTINGS = [(1, 5), (2, 13)]       # of the planes 8192 x 3 and 3 x 8192


def to_struct(F, m):
    """The settings as the package's DepthMedian."""
    return None if m is None else F.DepthMedian(*m)


def windows(A, radius):
    """The (2r+1)^2 planes of A seen from every offset of the window, int64; -1 where that pixel lies outside the image"""
    A = np.asarray(A)
    assert A.dtype == np.uint16 and A.ndim == 2
    h, w = A.shape
    r = int(radius)
    P = np.full((h + 2 * r, w + 2 * r), -1, np.int64)
    P[r:r + h, r:r + w] = A
    return np.stack([P[r + dy:r + dy + h, r + dx:r + dx + w] for dy in range(-r, r + 1) for dx in range(-r, r + 1)])


def finish(A, B):
    """(B uint16, MEDIAN uint8, the number of CHANGED pixels, the number of FILLED ones) of the contract"""
    A = np.asarray(A)
    B = np.asarray(B).astype(np.uint16)
    flags = np.where((A != 0) & (B != A), CHANGED, 0) + np.where((A == 0) & (B != 0), FILLED, 0)
    return B, flags.astype(np.uint8), int(np.count_nonzero(flags == CHANGED)), int(np.count_nonzero(flags == FILLED))


def median(A, m):
    """The contract on a whole plane: (B, MEDIAN, changed, filled)"""
    A = np.asarray(A)
    radius, fill_min = m
    W = windows(A, radius)
    member = W > 0                                    # inside the image and with a depth
    n = member.sum(axis=0)
    keys = np.sort(np.where(member, W, 1 << 20), axis=0)      # the members in ascending order, the others behind them
    med = np.take_along_axis(keys, np.maximum((n - 1) >> 1, 0)[None], axis=0)[0]
    med = np.where(n > 0, med, 0)
    fill = (A == 0) & (fill_min > 0) & (n >= fill_min)
    return finish(A, np.where((A != 0) | fill, med, 0))


def median_loop(A, m):
    """The same, pixel by pixel in the words of the contract (slow: small planes only)"""
    A = np.asarray(A)
    radius, fill_min = m
    h, w = A.shape
    B = np.zeros((h, w), np.uint16)
    for y in range(h):
        for x in range(w):
            V = sorted(int(A[yy, xx]) for yy in range(y - radius, y + radius + 1) for xx in range(x - radius, x + radius + 1)
                       if 0 <= yy < h and 0 <= xx < w and A[yy, xx] != 0)
            n = len(V)
            if A[y, x] != 0:
                B[y, x] = V[(n - 1) >> 1]
            elif fill_min > 0 and n >= fill_min:
                B[y, x] = V[(n - 1) >> 1]
    return finish(A, B)


# ---- the planes made on purpose ------------------------------------------------------------------

def _rng(seed):
    return np.random.Generator(np.random.PCG64(7000 + seed))


def noise(w, h, holes, seed):
    """uniform over [1, 65535], a fraction `holes` of the pixels without a value"""
    rng = _rng(seed)
    A = rng.integers(1, 65535, (h, w), endpoint=True).astype(np.uint16)
    A[rng.random((h, w)) < holes] = 0
    return A


def choice(w, h, values, holes, seed):
    rng = _rng(seed)
    A = rng.choice(np.asarray(values, np.uint16), (h, w))
    A[rng.random((h, w)) < holes] = 0
    return np.ascontiguousarray(A.astype(np.uint16))


def ramp(w, h):
    return np.ascontiguousarray((1000 + 7 * np.arange(w)[None, :] + 300 * np.arange(h)[:, None]).astype(np.uint16))


def surface(w, h, seed, pinholes=0.05, salt=0.05):
    """the plane the filter is for: a smooth slanted surface, 1.2 to 2.4 m at 5000 units per metre, with single pixels
    without depth and single pixels far off the surface"""
    return spoil(smooth(w, h), seed, pinholes, salt)


def smooth(w, h):
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    return np.rint(6000 + 4000 * x / max(w - 1, 1) + 2000 * y / max(h - 1, 1) + 150 * np.sin(x / 9.0) * np.cos(y / 7.0))


def stepped(w, h, seed):
    """surface() with a box at 1.4 m in front of it: a depth step the filter keeps and a gate's jump test marks"""
    A = smooth(w, h)
    A[h // 3:h // 3 + 25, w // 2:w // 2 + 30] = 7000
    return spoil(A, seed)


def spoil(A, seed, pinholes=0.05, salt=0.05):
    """a depth plane with a fraction `salt` of its pixels at random depths and a fraction `pinholes` without one"""
    rng = _rng(seed)
    A = np.asarray(A).astype(np.int64)
    s = rng.random(A.shape) < salt
    A[s] = rng.integers(1500, 40000, int(s.sum()))
    A[rng.random(A.shape) < pinholes] = 0
    return np.ascontiguousarray(A.astype(np.uint16))


def _single():
    A = np.zeros((9, 9), np.uint16)
    A[4, 4] = 4321
    return A


DEGENERATE = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5)]       # width x height
_MADE = {
    "noise-holes": lambda: noise(67, 35, 0.4, 1),
    "noise-full": lambda: noise(67, 35, 0.0, 2),
    "noise-sparse": lambda: noise(67, 35, 0.85, 3),
    "ties": lambda: choice(40, 33, (100, 101, 102), 0.3, 4),
    "extremes": lambda: choice(40, 33, (0, 1, 65534, 65535), 0.0, 5),
    "ramp": lambda: ramp(33, 17),
    "single": _single,
    "empty": lambda: np.zeros((9, 9), np.uint16),
    "surface": lambda: surface(130, 70, 6),
}
# (the seeds of the small planes: the first from 10 on at which the plane has two CHANGED pixels at every setting and
# two FILLED ones at some, which tests/test_fe_median_cpu.py asserts.  2 x 2 cannot have both: two CHANGED pixels need
# three pixels with a depth -- of two values the smaller is the lower median and stays -- and that leaves one to fill;
# its seed gives three values and one hole)
_DEGENERATE_SEEDS = {(1, 1): 10, (1, 9): 11, (9, 1): 11, (2, 2): 11, (3, 5): 10}
for _w, _h in DEGENERATE:
    _MADE["noise-holes-%dx%d" % (_w, _h)] = (lambda w=_w, h=_h: noise(w, h, 0.4, _DEGENERATE_SEEDS[(w, h)]))
MADE_NAMES = list(_MADE)
# what cannot change, or cannot be filled, by what it is: the conditions of the CPU test leave these out
NOTHING_TO_SHOW = ("ramp", "single", "empty", "noise-holes-1x1")
WITHOUT_HOLES = ("noise-full",)      # FILLED needs a pixel without depth: a plane without one has none at any setting
ONE_HOLE = ("noise-holes-2x2",)      # ... and this one has one (see the seeds above)
_CACHE = {}


def plane(name):
    if ("plane", name) not in _CACHE:
        A = _MADE[name]()
        A.setflags(write=False)
        _CACHE[("plane", name)] = A
    return _CACHE[("plane", name)]


def made(name, m):
    """(A, B, MEDIAN, changed, filled) of a made plane at the settings m, computed once and left unchanged"""
    key = (name, tuple(m))
    if key not in _CACHE:
        A = plane(name)
        B, flags, changed, filled = median(A, m)
        B.setflags(write=False)
        flags.setflags(write=False)
        _CACHE[key] = (A, B, flags, changed, filled)
    return _CACHE[key]


def long_plane(w, h):
    """8192 x 3 and 3 x 8192: the size limits, and a seam every 64 (16) pixels in one direction"""
    return noise(w, h, 0.4, 20 + (w > h))


def bad_medians():
    """Settings cvo_fe_check_depth_median refuses, one rule each: (radius, fill_min, pad_)"""
    return [(0, 0, 0), (3, 0, 0), (-1, 0, 0), (1, -1, 0), (1, 9, 0), (2, 25, 0), (2, -1, 0), (1, 0, 1), (2, 13, -1)]


def good_medians():
    """... and settings at the edge of what it accepts"""
    return [(1, 0, 0), (1, 8, 0), (2, 0, 0), (2, 24, 0)]
