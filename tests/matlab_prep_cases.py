"""The edge cases of the MATLAB cloud preparation (no test in here): inputs for cvo_hip_range_filter_grid_average
(csrc/cvo_prep.hip) and for its numpy oracle (oracle/matlab_prep.py).  tests/test_data.py writes down what the oracle
must answer on them, tests/test_gpu_matlab_edges.py holds the device to the oracle bit for bit.

A case is (label, xyz float32 n x 3, rgb uint8 n x 3, max_range, min_range, grid_size)."""
import numpy as np

F32 = np.float32
FAR = np.array([800.0, -1200.0, 600.0])
SUM_ORDER_SEED = 20            # the seed of the search in sum_order_points()


def expected(mp, xyz, rgb, max_range, min_range, grid_size):
    """What include/cvo_hip.h documents, from the oracle's two steps (mp = oracle.matlab_prep): non-finite points are
    dropped whatever the filter, max_range <= 0 switches the range filter off, a grid_size that is not > 0
    switches the downsampling off (the kept points in their order)."""
    xyz, rgb = np.asarray(xyz, F32), np.asarray(rgb, np.uint8)
    ok = np.isfinite(xyz).all(1)
    xyz, rgb = xyz[ok], rgb[ok]
    if max_range > 0:
        xyz, rgb = mp.pc_range_filter(xyz, rgb, max_range, min_range)
    if grid_size > 0:
        return mp.grid_average(xyz, rgb, grid_size)
    return xyz, rgb


def _blob(rng, n):
    xyz = (rng.normal(size=(n, 3)) * [1.5, 1.0, 0.7] + [0.2, -0.1, 2.0]).astype(F32)
    return xyz, rng.integers(0, 256, (n, 3)).astype(np.uint8)


NONFINITE_ROWS = ((0, 0, np.nan), (3, 1, np.inf), (77, 2, -np.inf), (200, 0, np.inf), (201, 1, np.nan), (499, 2, np.nan),
                  (300, 0, -np.inf), (300, 1, np.inf), (300, 2, np.nan))


def nonfinite():
    """500 points, seven of them with NaN / +Inf / -Inf coordinates (the first and the last among them)."""
    xyz, rgb = _blob(np.random.default_rng(41), 500)
    for row, col, v in NONFINITE_ROWS:
        xyz[row, col] = v
    return [("nonfinite range=%g grid=%g" % (rmax, grid), xyz, rgb, rmax, 0.8, grid)
            for rmax in (4.0, 0.0) for grid in (0.05, 0.0)]


RANGE_MAX, RANGE_MIN = 5.0, 0.75
RANGE_KEPT = (0, 1, 2, 3, 4, 5, 6, 7)   # rows of range_points() whose float32 range is inside [0.75, 5]; 8 ... 13 are one step outside


def range_points():
    up, down = (lambda v: np.nextafter(F32(v), F32(np.inf))), (lambda v: np.nextafter(F32(v), F32(0)))
    xyz = np.array([[0, 3, 4], [3, 4, 0], [-5, 0, 0], [0, 0, 0.75], [0.75, 0, 0], [0, -0.75, 0], [1, 1, 1],
                    [up(3), 4, 0],      # (longer than 5 in exact arithmetic; its float32 range rounds to 5: kept)
                    [0, 3, up(4)], [3, up(4), 0], [-up(5), 0, 0], [0, 0, down(0.75)], [down(0.75), 0, 0], [0, -down(0.75), 0]], F32)
    rgb = (np.arange(3 * len(xyz)).reshape(-1, 3) * 5).astype(np.uint8)
    return xyz, rgb


def range_limits():
    xyz, rgb = range_points()
    return [("limits kept", xyz, rgb, RANGE_MAX, RANGE_MIN, 0.0),
            ("min above max", xyz, rgb, RANGE_MIN, RANGE_MAX, 0.0),
            ("max_range 0, min_range 5", xyz, rgb, 0.0, RANGE_MAX, 0.0),
            ("max_range -1, min_range 5", xyz, rgb, -1.0, RANGE_MAX, 0.0)]


def sum_order_points():
    """32 points of a uniform cloud (seed SUM_ORDER_SEED) whose float32 range depends on the order of the sum:
    (xyz 32 x 3, r as (x*x + y*y) + z*z, r as x*x + (y*y + z*z))."""
    rng = np.random.default_rng(SUM_ORDER_SEED)
    p = rng.uniform(-3.0, 3.0, (2000, 3)).astype(F32)
    sq = (p * p).astype(F32)
    r_spec = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)).astype(F32)
    r_other = np.sqrt((sq[:, 0] + (sq[:, 1] + sq[:, 2]).astype(F32)).astype(F32)).astype(F32)
    pick = np.flatnonzero(r_spec != r_other)[:32]
    return p[pick], r_spec[pick], r_other[pick]


def sum_order():
    """Per point: max_range = min_range = its range in the specified order -- only that order keeps it."""
    xyz, r_spec, _ = sum_order_points()
    rgb = (np.arange(96).reshape(32, 3) * 2).astype(np.uint8)
    return [("sum order %d" % i, xyz, rgb, float(r_spec[i]), float(r_spec[i]), 0.0) for i in range(32)]


FACE_ORIGINS = {"near": np.array([0.25, -1.0, 0.5]), "far": np.array([0.25, -1.0, 0.5]) + FAR, "negative": np.array([-7.0, -9.0, -5.0])}


def face_points(origin, grid, n=600, seed=43):
    """Coordinates origin + k * grid (k < 40), a third of them as they are, a third one float32 step up, a third
    one step down: (xyz, k int n x 3, nudge in {-1, 0, 1} n x 3).  The first row is the origin itself and nothing
    steps below the lowest face, so the grid's anchor is the origin."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 40, (n, 3))
    nudge = rng.integers(-1, 2, (n, 3))
    k[0], nudge[0] = 0, 0
    nudge = np.where((k == 0) & (nudge < 0), 0, nudge)
    x = (origin + k * grid).astype(F32)
    x = np.where(nudge > 0, np.nextafter(x, F32(np.inf)), np.where(nudge < 0, np.nextafter(x, F32(-np.inf)), x)).astype(F32)
    return x, k, nudge


def voxel_faces():
    out = []
    for grid in (0.0625, 0.05):
        for name in ("near", "far", "negative"):
            xyz = face_points(FACE_ORIGINS[name], grid)[0]
            rgb = np.random.default_rng(44).integers(0, 256, (len(xyz), 3)).astype(np.uint8)
            out.append(("faces %s grid=%g" % (name, grid), xyz, rgb, 0.0, 0.0, grid))
    return out


def wide_keys():
    """3000 points in a 3 m box: 3001^3 voxels of 1 mm (keys above 2^32), 300001^3 of 10 um (above 2^53, below 2^62)."""
    rng = np.random.default_rng(45)
    xyz = rng.uniform(0.0, 3.0, (3000, 3))
    xyz[0], xyz[1] = 0.0, 3.0
    xyz = (xyz + [-1.0, 0.5, 2.0]).astype(F32)
    rgb = rng.integers(0, 256, (3000, 3)).astype(np.uint8)
    return [("keys above 2^32", xyz, rgb, 0.0, 0.0, 1e-3), ("keys above 2^53", xyz, rgb, 0.0, 0.0, 1e-5)]


def refused():
    """The box of wide_keys() in voxels of 1 um: 3000001^3 = 2.7e19 >= 2^63."""
    label, xyz, rgb, _, _, _ = wide_keys()[0]
    return [("2^63 voxels or more", xyz, rgb, 0.0, 0.0, 1e-6), ("far more", xyz, rgb, 0.0, 0.0, 1e-12)]


HEAVY_N = 70000
HEAVY_COLOUR = (101, 255, 0)     # means 100.5, 254.5 and 0.49


def heavy_voxels():
    """70 000 points in the voxel at the minimum corner (more than a 16-bit count), then 300 voxels of one point;
    the heavy voxel's colours alternate so that its means end in .5 (and 0.49)."""
    rng = np.random.default_rng(46)
    heavy = rng.uniform(0.05, 0.95, (HEAVY_N, 3))
    heavy[0] = 0.0
    i = np.arange(300)
    single = np.stack([1.5 + i % 20, 0.5 + i // 20, np.full(300, 0.5)], 1)
    xyz = np.concatenate([heavy, single])
    rgb = np.zeros((HEAVY_N + 300, 3), np.uint8)
    j = np.arange(HEAVY_N)
    rgb[:HEAVY_N, 0] = 100 + j % 2
    rgb[:HEAVY_N, 1] = 254 + (j + 1) % 2
    rgb[:HEAVY_N, 2] = (j % 100) < 49
    rgb[HEAVY_N:] = rng.integers(0, 256, (300, 3))
    perm = rng.permutation(len(xyz))      # the voxel's points lie scattered through the cloud
    perm = np.concatenate([[0], perm[perm != 0]])
    cases = [("70000 in one voxel", xyz[perm].astype(F32), rgb[perm], 0.0, 0.0, 1.0)]
    xyz, rgb = _blob(rng, 3000)
    cases.append(("one voxel of 100 m", xyz, rgb, 0.0, 0.0, 100.0))
    cases.append(("one point", xyz[:1], rgb[:1], 4.0, 0.8, 0.05))
    lone = np.full((40, 3), 9.0, F32)
    lone[17] = [0.5, -0.5, 2.0]
    cases.append(("one kept of forty", lone, rgb[:40], 4.0, 0.8, 0.05))
    return cases


def arena():
    """A large call, a small one, the large one again: the device arena is kept between calls."""
    rng = np.random.default_rng(47)
    big = _blob(rng, 100000)
    small = _blob(rng, 200)
    return [("100000", big[0], big[1], 4.0, 0.8, 0.05), ("200 after 100000", small[0], small[1], 4.0, 0.8, 0.05),
            ("100000 again", big[0], big[1], 4.0, 0.8, 0.05)]


def switches():
    xyz, rgb = _blob(np.random.default_rng(48), 300)
    return [("grid %r" % g, xyz, rgb, 4.0, 0.8, g) for g in (0.0, -0.05, float("nan"))] + \
           [("no points", np.zeros((0, 3), F32), np.zeros((0, 3), np.uint8), 4.0, 0.8, 0.05)]


GROUPS = {"nonfinite": nonfinite, "range_limits": range_limits, "sum_order": sum_order, "voxel_faces": voxel_faces,
          "wide_keys": wide_keys, "heavy_voxels": heavy_voxels, "arena": arena, "switches": switches}
