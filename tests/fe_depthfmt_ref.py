"""The depth-format contract of include/cvo_frontend.h (at CVO_FE_DEPTH_*) restated in numpy, and the inputs the tests of
it share.  Every operation is one float32 numpy operation, in the contract's order; numpy on the host keeps subnormals,
and the two `>= 2^-126` rules make that the same as a device that flushes them.

    v = the value (a float16 is widened exactly)
    no depth (0) unless v is finite and v >= 2^-126
    t = v * unit;          no depth unless t >= 2^-126
    q = rint(t * scale)    (ties to even)
    out = q if 1 <= q <= 65535 else 0

tests/test_fe_depthfmt_cpu.py shows which wrong versions (tests/fe_depthfmt_mutants.py) the inputs below tell from it;
tests/test_gpu_fe_depth_format.py holds k_fe_depth_convert to it by bytes on the same inputs."""
import numpy as np

U16, F32, F16 = 0, 1, 2
NAMES = ("U16", "F32", "F16")
FLOATS = (F32, F16)
DTYPES = {U16: np.uint16, F32: np.float32, F16: np.float16}
TINY = np.float32(2.0 ** -126)
f32 = np.float32


def widen(plane, fmt):
    """the plane's values as float32, exactly"""
    a = np.asarray(plane)
    assert a.dtype == DTYPES[fmt] and fmt in FLOATS, (a.dtype, fmt)
    return a.astype(np.float32)


def convert(plane, fmt, unit, scale):
    """the contract: a float plane -> uint16"""
    if fmt == U16:
        assert f32(unit) == f32(1.0)
        return np.asarray(plane, np.uint16).copy()
    with np.errstate(all="ignore"):
        v = widen(plane, fmt)
        ok = np.isfinite(v) & (v >= TINY)
        t = v * f32(unit)
        assert t.dtype == np.float32
        ok &= t >= TINY
        q = np.rint(t * f32(scale))
        assert q.dtype == np.float32
        ok &= (q >= f32(1.0)) & (q <= f32(65535.0))
        return np.where(ok, q, f32(0.0)).astype(np.uint16)


def frame_scale(colour_scale, rig_scale=None):
    """`scale` of the contract for a frame: of whatever reads the uploaded depth image first -- the depth camera's while
    one is set, otherwise the colour camera's in force"""
    return f32(colour_scale if rig_scale is None else rig_scale)


def check(fmt, unit):
    """what cvo_fe_check_depth_format accepts"""
    unit = f32(unit)
    if fmt not in (U16, F32, F16) or not np.isfinite(unit):
        return False
    if fmt == U16:
        return unit == f32(1.0)
    return f32(2.0 ** -20) <= unit <= f32(2.0 ** 20)


# ---- the named inputs --------------------------------------------------------------------------------
# name -> (unit, scale, the values and what the contract gives for each as float32; None: not stated here)
_NAN, _INF = float("nan"), float("inf")
NAMED = {
    # scale 5000, metres: the worked values of the contract, and everything that is no depth
    "tum": (1.0, 5000.0, (
        (0.8, 4000), (0.7998, 3999), (_NAN, 0), (_INF, 0), (-_INF, 0), (0.0, 0), (-0.0, 0), (-0.8, 0), (-1.5, 0),
        (1e-40, 0), (2.0 ** -149, 0), (-(2.0 ** -149), 0), (2.0 ** -126, 0), (0.0001, 0), (0.0003, 2), (0.0002, 1),
        (13.107, 65535), (13.1072, 0), (13.10711, 0), (1e30, 0), (3.4e38, 0), (1.0, 5000), (2.5, 12500))),
    # scale 1024: ties to even at both ends of the range
    "ties": (1.0, 1024.0, (
        (62.5 / 1024, 62), (63.5 / 1024, 64), (0.5 / 1024, 0), (1.5 / 1024, 2), (65534.5 / 1024, 65534), (65535.5 / 1024, 0),
        (1.0 / 1024, 1), (65535.0 / 1024, 65535), (65536.0 / 1024, 0), (2.5 / 1024, 2), (3.5 / 1024, 4), (0.75 / 1024, 1),
        (0.25 / 1024, 0), (-62.5 / 1024, 0))),
    # float millimetres at scale 5000: the order of the two multiplications shows
    "mm": (0.001, 5000.0, (
        (2947.099853515625, 14736), (800.0, 4000), (799.8, 3999), (13107.0, 65535), (13108.0, 0), (0.2, 1), (0.05, 0),
        (-800.0, 0), (_NAN, 0), (_INF, 0))),
    # a scale of 2^127: a subnormal value would reach the range if it were admitted
    "huge": (1.0, 2.0 ** 127, (
        (2.0 ** -127, 0), (1.5 * 2.0 ** -127, 0), (2.0 ** -126, 2), (1.5 * 2.0 ** -126, 3), (2.0 ** -149, 0), (2.0 ** -112, 32768),
        (2.0 ** -111, 0), (-(2.0 ** -126), 0), (0.0, 0))),
    # ... and a unit of 2^-20 under it: a subnormal product would
    "huge-unit": (2.0 ** -20, 2.0 ** 127, (
        (2.0 ** -107, 0), (1.5 * 2.0 ** -107, 0), (2.0 ** -106, 2), (2.0 ** -92, 32768), (2.0 ** -127, 0), (2.0 ** -91, 0))),
}
CONFIGS = tuple(NAMED)
ORDER_VALUE = 2947.099853515625   # of "mm": 14736 by the contract, 14735 by v * (unit * scale)


def named_values(config):
    unit, scale, rows = NAMED[config]
    return f32(unit), f32(scale), np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.int64)


def special_plane(config, fmt, w, h):
    """(plane, unit, scale): the config's named values, repeated row-major over w x h, in the format's dtype"""
    unit, scale, vals, _ = named_values(config)
    with np.errstate(all="ignore"):
        plane = np.resize(vals, (h, w)).astype(DTYPES[fmt])
    return plane, unit, scale


def random_plane(fmt, w, h, seed=5):
    """(plane, unit, scale): metres between 0.05 and 14.5 at scale 5000 -- both ends of the range are crossed -- with one
    value in sixteen without depth (zero, negative, NaN)"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    v = rng.uniform(0.05, 14.5, (h, w)).astype(np.float32)
    hole = rng.integers(0, 48, (h, w))
    v[hole == 0] = 0.0
    v[hole == 1] = -v[hole == 1]
    v[hole == 2] = np.nan
    return v.astype(DTYPES[fmt]), f32(1.0), f32(5000.0)


def all_patterns():
    """(plane, unit, scale): all 65536 float16 bit patterns as one 256 x 256 plane, as float millimetres at scale 5000"""
    return np.arange(65536, dtype=np.uint16).view(np.float16).reshape(256, 256), f32(0.001), f32(5000.0)


# (w, h, values between the end of a row and the next row): the vector path, its fallback and the row tail
SHAPES = ((1, 1, 0), (5, 3, 0), (5, 3, 1), (63, 2, 0), (64, 2, 0), (65, 3, 0), (67, 5, 0), (259, 2, 0),
          (64, 2, 1), (64, 3, 3), (8, 4, 2), (12, 3, 5))


def cases(fmt):
    """(w, h, pad in values, kind) of the stand-alone GPU test: kind is "random", a config of NAMED, or "all-patterns" """
    out = []
    for w, h, pad in SHAPES:
        out.append((w, h, pad, "random"))
        out += [(w, h, pad, c) for c in CONFIGS]
    if fmt == F16:
        out.append((256, 256, 0, "all-patterns"))
    return out


def make_input(fmt, w, h, kind):
    if kind == "random":
        return random_plane(fmt, w, h)
    if kind == "all-patterns":
        assert fmt == F16 and (w, h) == (256, 256)
        return all_patterns()
    return special_plane(kind, fmt, w, h)


def padded(plane, pad, fill=0x5A):
    """(the buffer, its pitch in bytes): the plane's rows `pad` values further apart, the gap filled with a byte"""
    h, w = plane.shape
    item = plane.dtype.itemsize
    buf = np.full((h, (w + pad) * item), fill, np.uint8)
    buf[:, :w * item] = np.ascontiguousarray(plane).view(np.uint8).reshape(h, w * item)
    return buf, (w + pad) * item


# the depth camera of the frame tests: a scale of its own beside a colour camera of the table (TUM fr1: 5000)
RIG_CASE = {"colour_scale": 5000.0, "rig_scale": 1000.0, "width": 80, "height": 60}


def metres(depth_u16, scale, fmt=F32):
    """a uint16 depth image as the float plane a network would hand over: (float32)d / scale, then the format's dtype"""
    with np.errstate(all="ignore"):
        return (np.asarray(depth_u16).astype(np.float32) / f32(scale)).astype(DTYPES[fmt])
