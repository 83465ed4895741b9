"""The binning contract of include/cvo_frontend.h (at cvo_fe_binning), restated in numpy: what k_fe_bin of
csrc/cvo_bin.hip is held to by bytes, and what the working camera of cvo_fe_bin_camera / cvo_fe_bin_stereo_rig is held
to by bits.  Colour by int64 block sums; depth by sorting keys with "none" last and picking (k - 1) >> 1; the cameras
in np.float32, one operation at a time.  cases() are the sizes and inputs the stand-alone entries are run on; which
wrong versions of the stage they tell from this one is asserted in tests/test_fe_binning_cpu.py
(tests/fe_binning_mutants.py)."""
import numpy as np

FACTORS = (2, 3, 4)
NONE_KEY = 1 << 16   # behind every depth, 65535 included


def check(binning, width, height):
    """cvo_fe_check_binning: binning is (factor, depth_min, pad_) or None; width x height the working size"""
    if binning is None:
        return False
    f, dmin, pad = binning
    if f not in FACTORS or pad != 0 or width < 1 or height < 1:
        return False
    return 1 <= dmin <= f * f and f * width <= 8192 and f * height <= 8192


def blocks(plane, f):
    """an (fh, fw, ...) array as (h, w, f*f, ...): member j*f + i of block (x, y) is input pixel (fx + i, fy + j)"""
    fh, fw = plane.shape[:2]
    assert fh % f == 0 and fw % f == 0
    h, w = fh // f, fw // f
    rest = plane.shape[2:]
    b = plane.reshape((h, f, w, f) + rest)
    b = np.moveaxis(b, 1, 2)                      # h, w, f (j), f (i), ...
    return b.reshape((h, w, f * f) + rest)


def bin_colour(bgr, f):
    """(S + (n >> 1)) // n per channel, S the sum of the block's n bytes"""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    n = f * f
    s = blocks(bgr, f).astype(np.int64).sum(axis=2)
    return ((s + (n >> 1)) // n).astype(np.uint8)


def bin_depth(plane, f, depth_min):
    """the lower median of the block's non-zero values where there are at least depth_min of them, else 0"""
    plane = np.asarray(plane)
    assert plane.dtype == np.uint16 and plane.ndim == 2
    b = blocks(plane, f).astype(np.int64)
    key = np.sort(np.where(b == 0, NONE_KEY, b), axis=2)
    k = (b != 0).sum(axis=2)
    pick = np.maximum(k - 1, 0) >> 1
    med = np.take_along_axis(key, pick[..., None], axis=2)[..., 0]
    return np.where(k >= depth_min, med, 0).astype(np.uint16)


def _f32(x):
    return np.float32(x)


def bin_intrinsics(fx, fy, cx, cy, f):
    """fx / f, fy / f, (cx - c) / f, (cy - c) / f in float32, c = 0.5 * (f - 1), each operation rounded on its own"""
    ff = _f32(f)
    c = _f32(0.5) * _f32(f - 1)
    return (_f32(fx) / ff, _f32(fy) / ff, (_f32(cx) - c) / ff, (_f32(cy) - c) / ff)


def bin_camera(model, f):
    """model: (depth_scale, fx, fy, cx, cy, dist[5]); depth_scale and dist unchanged"""
    scale, fx, fy, cx, cy, dist = model
    return (_f32(scale),) + bin_intrinsics(fx, fy, cx, cy, f) + (tuple(_f32(d) for d in dist),)


def bin_lens(lens, f):
    """lens: (fx, fy, cx, cy, dist[5])"""
    fx, fy, cx, cy, dist = lens
    return bin_intrinsics(fx, fy, cx, cy, f) + (tuple(_f32(d) for d in dist),)


def bin_stereo_rig(rig, f):
    """rig: (left, right, R_left, R_right, fx, fy, cx, cy, baseline, depth_scale) as StereoRig.astuple() gives it"""
    left, right, rl, rr, fx, fy, cx, cy, baseline, scale = rig
    return ((bin_lens(left, f), bin_lens(right, f), tuple(_f32(v) for v in rl), tuple(_f32(v) for v in rr)) +
            bin_intrinsics(fx, fy, cx, cy, f) + (_f32(baseline), _f32(scale)))


# ---- the inputs of the stand-alone entries ------------------------------------------------------------

def sizes(f):
    """output sizes (w, h): tails, group and block seams with a tail, a square, and the longest row and column"""
    return ((1, 1), (2, 1), (3, 2), (5, 3), (13, 7), (66, 18), (130, 34), (64, 64), (8192 // f, 1), (1, 8192 // f))


COLOUR_KINDS = ("random", "zeros", "full", "checker", "ramps", "phases")
DEPTH_KINDS = ("half", "zeros", "full", "one", "edge", "extremes", "even")


def _phase_pixels(w, h):
    """working pixels beside a corner and beside a group seam (x = 3 | 4), inside w x h"""
    return [(x, y) for x, y in ((0, 0), (w - 1, h - 1), (3, 0), (4, h - 1), (min(w - 1, 7), 0)) if 0 <= x < w and 0 <= y < h]


def colour_input(f, w, h, kind, seed=5):
    """an (fh, fw, 3) uint8 image; "phases": a list of them, a single 255 at each of the f*f block phases"""
    fw, fh = f * w, f * h
    rng = np.random.RandomState(seed + 31 * f + w + 7 * h)
    if kind == "random":
        return rng.randint(0, 256, (fh, fw, 3)).astype(np.uint8)
    if kind == "zeros":
        return np.zeros((fh, fw, 3), np.uint8)
    if kind == "full":
        return np.full((fh, fw, 3), 255, np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:fh, 0:fw]
        return np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    if kind == "ramps":
        yy, xx = np.mgrid[0:fh, 0:fw]
        return np.stack([(xx * (c + 1) + yy * (3 * c + 5) + 11 * c) & 255 for c in range(3)], axis=2).astype(np.uint8)
    assert kind == "phases"
    out = []
    for j in range(f):
        for i in range(f):
            img = np.zeros((fh, fw, 3), np.uint8)
            for q, (x, y) in enumerate(_phase_pixels(w, h)):
                img[f * y + j, f * x + i, q % 3] = 255
            out.append(img)
    return out


def depth_input(f, w, h, kind, depth_min, seed=9):
    """an (fh, fw) uint16 plane"""
    fw, fh = f * w, f * h
    n = f * f
    rng = np.random.RandomState(seed + 31 * f + w + 7 * h + 3 * depth_min)
    if kind == "half":
        d = rng.randint(1, 65536, (fh, fw))
        return np.where(rng.rand(fh, fw) < 0.5, 0, d).astype(np.uint16)
    if kind == "zeros":
        return np.zeros((fh, fw), np.uint16)
    if kind == "full":
        return np.full((fh, fw), 65535, np.uint16)
    b = np.zeros((h, w, n), np.int64)
    if kind == "one":                             # one valid pixel per block, the phase moving from block to block
        yy, xx = np.mgrid[0:h, 0:w]
        np.put_along_axis(b, ((xx + 3 * yy) % n)[..., None], rng.randint(1, 65536, (h, w, 1)), axis=2)
    elif kind == "edge":                          # exactly depth_min - 1 and depth_min valid, alternating, at random phases
        yy, xx = np.mgrid[0:h, 0:w]
        count = depth_min - ((xx + yy) & 1)
        order = np.argsort(rng.rand(h, w, n), axis=2)
        vals = rng.randint(1, 65536, (h, w, n))
        b = np.where(order < count[..., None], vals, 0)
    elif kind == "extremes":                      # only 1 and 65535, any count
        b = rng.choice(np.array([0, 1, 65535]), (h, w, n))
    else:
        assert kind == "even"                     # an even count of distinct values: lower and upper median differ
        yy, xx = np.mgrid[0:h, 0:w]
        count = 2 * (1 + (xx + yy) % (n // 2))
        order = np.argsort(rng.rand(h, w, n), axis=2)
        vals = np.argsort(rng.rand(h, w, n), axis=2) * 1000 + 40000   # (above 32767: signed 16-bit keys would misorder)
        vals[..., 0] = 7
        b = np.where(order < count[..., None], vals, 0)
    plane = np.moveaxis(b.reshape(h, w, f, f), 2, 1).reshape(fh, fw)
    return plane.astype(np.uint16)


def depth_mins(f):
    return (1, f * f // 2, f * f)


def cases():
    """(plane kind, f, w, h, input kind, depth_min or None): every input at the small sizes, random at the long ones"""
    out = []
    for f in FACTORS:
        for w, h in sizes(f):
            long_ = max(w, h) > 200
            for kind in (("random",) if long_ else COLOUR_KINDS):
                out.append(("colour", f, w, h, kind, None))
            for dmin in depth_mins(f):
                for kind in (("half",) if long_ else DEPTH_KINDS):
                    out.append(("depth", f, w, h, kind, dmin))
    return out


def case_inputs(case):
    """the list of inputs of a case (one, but for "phases")"""
    plane, f, w, h, kind, dmin = case
    if plane == "colour":
        src = colour_input(f, w, h, kind)
        return src if isinstance(src, list) else [src]
    return [depth_input(f, w, h, kind, dmin)]
