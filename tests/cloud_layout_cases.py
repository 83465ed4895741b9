"""The clouds of tests/test_cloud_layout_cpu.py and tests/test_gpu_cloud_layout.py (no test in here): shapes
that stress the hand-over's arithmetic (csrc/cvo_cloud.hip) -- ties in every digit of the sort, zero / tiny /
overflowing extents, points exactly on the quantisation steps, a cloud far from the origin -- at the sizes
where the hand-over changes its way: a run of 64, the padding bucket of 256, the block of 1024 (waves with no
positions in the LDS sort), the one-launch limit of 16384.  Coordinates are made in float64 and rounded once."""
import numpy as np

FAR = np.array([800.0, -1200.0, 600.0])

ALL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16383, 16384, 16385, 20000)
EDGE_SIZES = (65, 1025, 16384, 16385)
EVERY_SIZE_SHAPES = ("synthetic", "synthetic_far")
EDGE_SHAPES = ("one_point", "eight_tiled", "lattice_tiled", "plane", "line", "tiny_extent", "overflow_extent",
               "exact_steps", "special_features")
CASES = [(s, n) for s in EVERY_SIZE_SHAPES for n in ALL_SIZES] + [(s, n) for s in EDGE_SHAPES for n in EDGE_SIZES]


def _features(rng, n):
    return (rng.normal(size=(n, 5)) * [80.0, 80.0, 80.0, 10.0, 10.0] + [120.0, 120.0, 120.0, 0.0, 0.0]).astype(np.float32)


def cloud(data, shape, n, which):
    """(xyz float32 n x 3, feat float32 n x 5) of `shape`; which = 0 / 1: the fixed / the moving cloud of a
    pair (same shape, other points or another order).  data: the package's data module (synthetic_pair)."""
    rng = np.random.default_rng(1000 * len(shape) + 7 * n + which)
    feat = _features(rng, n)
    if shape in ("synthetic", "synthetic_far", "special_features"):
        xyz = data.synthetic_pair(n, n, seed=300 + n % 97)[2 * which].astype(np.float64)
        if shape == "synthetic_far":
            xyz = xyz + FAR
        if shape == "special_features":
            special = np.array([-0.0, np.inf, -np.inf, 0.0], np.float32)
            hit = rng.random((n, 5)) < 0.3
            feat = np.where(hit, special[rng.integers(0, 4, (n, 5))], feat).astype(np.float32)
            feat[0] = [-0.0, np.inf, -np.inf, -0.0, -0.0]
            feat[n - 1] = [np.inf, -0.0, -0.0, -np.inf, np.inf]
    elif shape == "one_point":
        xyz = np.tile([[0.3, -1.7, 2.2]], (n, 1))
    elif shape == "eight_tiled":   # eight keys, each n / 8 times, interleaved: stability decides the order
        base = rng.uniform(-2.0, 2.0, (8, 3))
        xyz = np.tile(base, ((n + 7) // 8, 1))[:n]
    elif shape == "lattice_tiled":
        g = np.arange(4) * 0.5 - 0.4
        base = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(64, 3)[rng.permutation(64)]
        xyz = np.tile(base, ((n + 63) // 64, 1))[:n]
    elif shape == "plane":
        xyz = rng.uniform(-1.5, 1.5, (n, 3))
        xyz[:, 2] = 1.25
    elif shape == "line":
        xyz = rng.uniform(-1.5, 1.5, (n, 3))
        xyz[:, 1] = -0.5
        xyz[:, 2] = 1.25
    elif shape == "tiny_extent":   # 1e-30 m along y: 1023 / ext is 1e33, still finite
        xyz = rng.uniform(-1.5, 1.5, (n, 3))
        xyz[:, 1] = rng.integers(0, 1025, n) * (1e-30 / 1024)
        xyz[0, 1], xyz[1, 1] = 0.0, 1e-30
    elif shape == "overflow_extent":   # hi - lo overflows float32 along x: that axis gives no key bits
        xyz = rng.uniform(-1.5, 1.5, (n, 3))
        xyz[:, 0] = np.array([-3e38, -1e38, 1e38, 3e38])[rng.integers(0, 4, n)]
        xyz[0, 0], xyz[1, 0] = -3e38, 3e38
    elif shape == "exact_steps":   # extent 1023 on every axis, every coordinate on a step: (x - lo) * inv is an integer
        xyz = rng.integers(0, 1024, (n, 3)).astype(np.float64)
        xyz[0], xyz[1] = 0.0, 1023.0
        xyz += [-100.0, 7.0, 0.0]
    else:
        raise ValueError(shape)
    if which == 1 and shape not in ("synthetic", "synthetic_far", "special_features"):
        xyz = xyz[::-1]   # the moving cloud: the same points the other way round (ties resolve differently)
    return np.ascontiguousarray(xyz.astype(np.float32)), feat
