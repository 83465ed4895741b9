"""A numpy/Python restatement of the front end's speckle contract (include/cvo_frontend.h, at cvo_fe_speckle): the
components of a uint16 plane under "4-neighbours whose values differ by max_diff at the most", their pixel counts
(SIZE) and what the filter changes.  Two statements that share no code: a union-find over the joined pairs
(components) and a breadth-first flood fill (flood); tests/test_fe_speckle_cpu.py holds them equal.  Integer
arithmetic throughout; the kernels of csrc/cvo_speckle.hip are held to it by bytes.

Settings here are a pair (max_size, max_diff).  Also here: the planes made on purpose and the cases the tests share."""
from collections import deque

import numpy as np

SPECKLE = 32               # CVO_FE_STEREO_SPECKLE
MAX_SIZE, MAX_DIFF = 1 << 26, 65535


def to_struct(F, sp):
    """The settings as the package's Speckle."""
    return None if sp is None else F.Speckle(*sp)


# ---- the contract ----------------------------------------------------------------------------------

def joined_pairs(q, max_diff):
    """The joined pairs (a, b) of flat indices, b the left or the upper neighbour of a."""
    q = np.asarray(q)
    h, w = q.shape
    v = q.astype(np.int64)                                  # the difference is of signed integers
    idx = np.arange(h * w).reshape(h, w)
    hor = (v[:, 1:] != 0) & (v[:, :-1] != 0) & (np.abs(v[:, 1:] - v[:, :-1]) <= max_diff)
    ver = (v[1:, :] != 0) & (v[:-1, :] != 0) & (np.abs(v[1:, :] - v[:-1, :]) <= max_diff)
    a = np.concatenate([idx[:, 1:][hor], idx[1:, :][ver]])
    b = np.concatenate([idx[:, :-1][hor], idx[:-1, :][ver]])
    return a, b


def sizes_of_pairs(q, a, b):
    """SIZE of the plane q whose joined pairs are (a, b): a union-find with path halving"""
    q = np.asarray(q)
    n = q.size
    parent = list(range(n))
    for x, y in zip(a.tolist(), b.tolist()):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        while parent[y] != y:
            parent[y] = parent[parent[y]]
            y = parent[y]
        if x != y:
            if x < y:
                x, y = y, x
            parent[x] = y
    p = np.array(parent, np.int64)
    while True:                                             # every pixel to its root
        pp = p[p]
        if np.array_equal(pp, p):
            break
        p = pp
    count = np.bincount(p, minlength=n)
    return np.where(q.reshape(-1) != 0, count[p], 0).astype(np.uint32).reshape(q.shape)


def components(q, max_diff):
    """SIZE: h x w uint32, the pixel count of every valid pixel's component and 0 where q == 0"""
    return sizes_of_pairs(q, *joined_pairs(q, max_diff))


def flood(q, max_diff, against_first=False):
    """SIZE by breadth-first flood fills in scan order; nothing shared with components().  (`against_first` is a
    mutant: the difference is taken against the fill's first pixel, not the neighbour.)"""
    q = np.asarray(q)
    h, w = q.shape
    v = q.astype(np.int64).tolist()
    size = np.zeros((h, w), np.uint32)
    seen = [[False] * w for _ in range(h)]
    for y0 in range(h):
        for x0 in range(w):
            if v[y0][x0] == 0 or seen[y0][x0]:
                continue
            seen[y0][x0] = True
            members, todo = [(y0, x0)], deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                ref = v[y0][x0] if against_first else v[y][x]
                for yn, xn in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= yn < h and 0 <= xn < w and not seen[yn][xn] and v[yn][xn] != 0 and abs(v[yn][xn] - ref) <= max_diff:
                        seen[yn][xn] = True
                        members.append((yn, xn))
                        todo.append((yn, xn))
            ys, xs = zip(*members)
            size[list(ys), list(xs)] = len(members)
    return size


def filter_plane(q, sp, sizes=None):
    """cvo_fe_filter_speckles: (the filtered plane, SIZE, the number of pixels zeroed)"""
    q = np.asarray(q)
    sizes = components(q, sp[1]) if sizes is None else sizes
    gone = (q != 0) & (sizes <= sp[0])
    return np.where(gone, 0, q).astype(np.uint16), sizes, int(np.count_nonzero(gone))


def apply(q, flags, depth, sp):
    """What the filter changes of a stereo frame: (disparity, flags, depth, SIZE)"""
    out, sizes, _ = filter_plane(q, sp)
    gone = out != np.asarray(q)
    return (out, (np.asarray(flags) | np.where(gone, SPECKLE, 0)).astype(np.uint8),
            np.where(gone, 0, depth).astype(np.uint16), sizes)


def frame(P, sp):
    """the planes of a stereo frame (fe_stereo_ref.match()'s, or a rig frame's) behind the filter, and `sizes`"""
    disparity, flags, depth, sizes = apply(P["disparity"], P["flags"], P["depth"], sp)
    return dict(P, disparity=disparity, flags=flags, depth=depth, sizes=sizes)


def census_of_sizes(sizes):
    """the sizes of the components, largest first"""
    s = np.asarray(sizes).reshape(-1)
    s = s[s != 0]
    vals, counts = np.unique(s, return_counts=True)
    out = []
    for v, c in zip(vals.tolist(), counts.tolist()):
        assert c % v == 0
        out += [v] * (c // v)
    return sorted(out, reverse=True)


# ---- the planes made on purpose --------------------------------------------------------------------------

def serpentine(w, h, value=500):
    """Even rows valid throughout, odd rows at one end only, the ends alternating: ONE component, one pixel wide where it
    turns, that crosses every border of a tiling of any tile size.  Returns (plane, its size)."""
    q = np.zeros((h, w), np.uint16)
    q[0::2, :] = value
    q[1::4, w - 1] = value
    q[3::4, 0] = value
    return q, ((h + 1) // 2) * w + h // 2


def ramp(w, h, step):
    """q = 16 + x * step: one component of w * h pixels under max_diff = step, w columns of h under step - 1"""
    assert 16 + (w - 1) * step <= 65535
    return np.ascontiguousarray(np.broadcast_to((16 + np.arange(w) * step).astype(np.uint16)[None, :], (h, w)))


def checker_valid(w, h, value=100):
    """valid pixels on a checkerboard: every component has one pixel; 8 neighbours would join them all"""
    return (value * ((np.arange(w)[None, :] + np.arange(h)[:, None]) % 2 == 0)).astype(np.uint16)


def extremes(w=8, h=4):
    """1 beside 65535: they differ by 65534 (a uint16 subtraction that wraps sees 2)"""
    q = np.full((h, w), 1, np.uint16)
    q[:, w // 2:] = 65535
    return q


LEVELS = (100, 140, 180)         # of blobs(): 40 apart, so that max_diff 16 joins pixels of one level only
BLOB_DIFF = 16


def blobs(w, h, seed):
    """PCG64 draws: a pixel is valid with probability 0.6, its value one of three levels.  Returns (plane, max_size):
    the smallest s for which components of exactly s and of exactly s + 1 pixels both occur under BLOB_DIFF."""
    rng = np.random.Generator(np.random.PCG64(seed))
    valid = rng.random((h, w)) < 0.6
    q = np.where(valid, np.array(LEVELS)[rng.integers(0, 3, (h, w))], 0).astype(np.uint16)
    have = set(census_of_sizes(components(q, BLOB_DIFF)))
    s = min(v for v in have if v + 1 in have)            # (fails where there is none)
    return q, s


SHAPES = [(64, 64), (127, 193), (257, 131), (1241, 64)]    # width, height: of serpentine and blobs
RAMP_STEP = 3


def made_planes():
    """name -> (plane, (max_size, max_diff)): every plane made on purpose with every setting it runs under"""
    out = {}
    for w, h in SHAPES:
        q, n = serpentine(w, h)
        out["serpentine-%dx%d-all" % (w, h)] = (q, (n, 0))
        out["serpentine-%dx%d-none" % (w, h)] = (q, (n - 1, 0))
        q, s = blobs(w, h, 900 + w)
        out["blobs-%dx%d" % (w, h)] = (q, (s, BLOB_DIFF))
    q = ramp(127, 193, RAMP_STEP)
    out["ramp-one"] = (q, (193, RAMP_STEP))                 # one component of 127 * 193: nothing goes
    out["ramp-columns"] = (q, (193, RAMP_STEP - 1))         # 127 columns of 193: everything goes
    out["ramp-columns-kept"] = (q, (192, RAMP_STEP - 1))    # ... and nothing
    out["checker"] = (checker_valid(127, 193), (1, 65535))
    out["extremes-joined"] = (extremes(), (16, MAX_DIFF))   # one component of 32: nothing goes
    out["extremes-apart"] = (extremes(), (16, 10))          # two of 16: everything goes
    out["1x1"] = (np.full((1, 1), 7, np.uint16), (1, 0))
    out["1x300"] = (serpentine(1, 300)[0], (299, 0))
    out["300x1"] = (serpentine(300, 1)[0], (300, 0))
    out["zero"] = (np.zeros((64, 96), np.uint16), (MAX_SIZE, MAX_DIFF))
    out["equal"] = (np.full((131, 257), 4242, np.uint16), (33666, 0))
    out["equal-all"] = (np.full((131, 257), 4242, np.uint16), (33667, 0))
    # the checkerboard with one bar through it: the bar's component is kept, the single pixels go
    q = checker_valid(64, 64).copy()
    q[20, :] = 100
    out["barred-checker"] = (q, (1, 65535))
    return out


# cases whose filter is all-or-nothing by design (every other case must change a pixel and keep one)
ALL_OR_NOTHING = ("serpentine-", "ramp-", "checker", "extremes-", "1x1", "1x300", "300x1", "zero", "equal")

_DONE = {}


def made(name):
    """(plane, settings, filtered plane, SIZE, removed) of a made plane: computed once, left unchanged"""
    if not _DONE:
        for n, (q, sp) in made_planes().items():
            out = (q, sp) + filter_plane(q, sp)
            for a in out:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            _DONE[n] = out
    return _DONE[name]


MADE_NAMES = sorted(made_planes())


# ---- the stereo cases behind the filter --------------------------------------------------------------

# name of a case of fe_stereo_paths_ref.inputs -> settings
STEREO_CASES = {"default-127x193-83": (100, 16), "d128": (8, 16), "noise": (12, 16), "flat": (12, 16), "wide": (100, 16)}
# settings alternating on one context (None: no filter), on two images of one size and one Stereo
ALTERNATING = (None, (12, 16), (100, 32), None, (12, 16))
ALTERNATING_IMAGES = ("default-96x64-82", "noise")
RIG_SPECKLE = (12, 16)                                   # under rig "B" of fe_stereo_rig_ref
GATE_CASE = ("default-127x193-82", (100, 16), 0x0F)      # behind a gate and a mask
PATHS8_CASE = ("default-127x193-83", (100, 16), 0xFF)    # another S, the same rule
_FRAMES = {}


def case_frame(name, sp, mask=0x0F):
    """frame() of a stereo case under a path mask: computed once, left unchanged"""
    import fe_stereo_paths_ref as P
    key = (name, tuple(sp), mask)
    if key not in _FRAMES:
        out = frame(P.case_planes(name, mask), sp)
        for a in out.values():
            a.setflags(write=False)
        _FRAMES[key] = out
    return _FRAMES[key]


def bad_speckles():
    """settings cvo_fe_check_speckle refuses"""
    return [(0, 16), (-1, 16), (MAX_SIZE + 1, 16), (12, -1), (12, 65536)]


def good_speckles():
    """... and settings at the edge of what it accepts"""
    return [(1, 0), (MAX_SIZE, MAX_DIFF)]
