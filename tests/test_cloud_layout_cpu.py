"""tests/cloud_layout_ref.py (what the device's cloud hand-over, csrc/cvo_cloud.hip, is held to in
tests/test_gpu_cloud_layout.py) against definitions and hand-written answers -- not against itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_layout_cases as cases  # noqa: E402
import cloud_layout_ref as ref  # noqa: E402

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _key_of_cells(q):
    """Morton key of integer cells (x lowest), written out bit by bit in Python integers."""
    key = 0
    for b in range(10):
        for a in range(3):
            key |= ((int(q[a]) >> b) & 1) << (3 * b + a)
    return key


def _keys_along(xyz, order):
    lo, hi = ref.bounding_box(xyz)
    return ref.morton_keys(xyz, lo, hi)[order]


@pytest.mark.parametrize("shape,n", cases.CASES)
def test_order_spheres_and_padding_follow_their_definitions(pkg, shape, n):
    """Every committed case: the order is a permutation with non-decreasing keys, equal keys in the caller's
    order; rows carry the caller's data; in float64 every live point lies inside its run's sphere; padding
    is parked more than 1 km from every real point, and the two pad axes park it in different places."""
    for which in (0, 1):
        xyz, feat = cases.cloud(pkg.data, shape, n, which)
        rows, pos, feat8, seg, bbox, order = ref.layout(xyz, feat, False, which)
        assert rows % 256 == 0 and 0 <= rows - n < 256
        assert pos.shape == (rows, 4) and feat8.shape == (rows, 8) and seg.shape == (rows // 64, 4)
        assert np.array_equal(np.sort(order), np.arange(n))
        k = _keys_along(xyz, order).astype(np.int64)
        assert np.all(np.diff(k) >= 0)
        tie = np.diff(k) == 0
        assert np.all(np.diff(order)[tie] > 0)
        assert np.array_equal(_bits(bbox), _bits(np.concatenate([xyz.min(0), xyz.max(0)])))
        # rows: the caller's data, by the caller's index
        idx = feat8[:n, 5].view(np.int32)
        assert np.array_equal(idx, order)
        assert np.array_equal(_bits(pos[:n, :3]), _bits(xyz[idx]))
        assert np.array_equal(_bits(pos[:n, 3]), _bits(feat[idx, 4]))
        assert np.array_equal(_bits(feat8[:n, :5]), _bits(feat[idx]))
        assert not feat8[:, 6:].any()
        # the same from column-major features
        other = ref.layout(xyz, np.ascontiguousarray(feat.T), True, which)
        for a, b in zip((pos, feat8, seg), other[1:4]):
            assert np.array_equal(_bits(a), _bits(b))
        # containment, in float64
        p64, s64 = pos[:n, :3].astype(np.float64), seg.astype(np.float64)
        run = np.arange(n) // 64
        d = np.sqrt(((p64 - s64[run, :3]) ** 2).sum(1))
        assert np.all(d <= s64[run, 3])
        # padding
        live_runs = (n + 63) // 64
        assert np.all(_bits(pos[n:, 3]) == 0x7FC00000) and np.all(_bits(feat8[n:, :5]) == 0x7FC00000)
        assert np.all(feat8[n:, 5].view(np.int32) == -1)
        for g in range(live_runs, rows // 64):
            c, r = s64[g, :3], s64[g, 3]
            assert np.sqrt(((p64 - c) ** 2).sum(1)).min() - r > 1000.0
            members = pos[g * 64:(g + 1) * 64, :3].astype(np.float64)
            assert np.all(np.sqrt(((members - c) ** 2).sum(1)) <= r)
        if rows > n:
            assert np.sqrt(((pos[n:, None, :3].astype(np.float64) - p64[None, ::max(1, n // 64)]) ** 2).sum(2)).min() > 1000.0
            flipped = ref.layout(xyz, feat, False, 1 - which)[1]
            assert np.array_equal(_bits(flipped[:n]), _bits(pos[:n]))
            assert np.all(flipped[n:, 1 - which] - pos[n:, 1 - which] >= 1.0e4)


@pytest.mark.parametrize("lo,ext", [((-100.0, 7.0, 0.0), 1023.0), ((-3.0, 0.5, 16.0), 2.0), ((0.0, -64.0, 1.0), 64.0)])
def test_keys_equal_an_independent_quantisation_on_an_exact_lattice(lo, ext):
    """Extents of 1023 (1023 / ext = 1: the points sit on the steps) and of a power of two: on a lattice of
    1 / 1024ths of the extent every float32 step of the key arithmetic is exact, so the cell is
    floor(j * 1023 / 1024) for lattice index j in integers."""
    rng = np.random.default_rng(5)
    n = 3000
    j = rng.integers(0, 1025, (n, 3))
    j[0], j[1] = 0, 1024
    j[2:12] = rng.integers(0, 2, (10, 3)) * 1024                          # corners
    step = 1023 if ext == 1023.0 else 1024
    j = np.minimum(j, step)
    j[1] = step
    xyz = (np.array(lo) + j * (ext / step)).astype(F32)
    assert np.array_equal(xyz.astype(np.float64), np.array(lo) + j * (ext / step))   # the lattice is exact in float32
    want = [_key_of_cells([(int(v) * 1023) // step for v in row]) for row in j]
    blo, bhi = ref.bounding_box(xyz)
    assert np.array_equal(ref.morton_keys(xyz, blo, bhi), np.array(want, np.uint32))
    order = ref.layout(xyz, np.zeros((n, 5), F32), False, 0)[5]
    assert sorted(zip(want, range(n))) == [(want[i], i) for i in order]


def test_spread_is_every_third_bit():
    assert ref.spread_bits(np.array([0, 1, 2, 1023, 0b1000000001], np.uint32)).tolist() == \
        [0, 1, 8, 0o1111111111, (1 << 27) | 1]


def test_three_points_by_hand():
    """n = 3, x in {0, 1023}, y in {7, 1030}, z constant: cells (0,0,0), (1023,0,0), (0,1023,0)."""
    xyz = np.array([[1023.0, 7.0, 2.0], [0.0, 1030.0, 2.0], [0.0, 7.0, 2.0]], F32)
    feat = np.arange(15, dtype=F32).reshape(3, 5)
    rows, pos, feat8, seg, bbox, order = ref.layout(xyz, feat, False, 1)
    assert rows == 256 and bbox.tolist() == [0.0, 7.0, 2.0, 1023.0, 1030.0, 2.0]
    kx, ky = 0o1111111111, 0o2222222222
    assert ref.morton_keys(xyz, bbox[:3], bbox[3:]).tolist() == [kx, ky, 0]
    assert order.tolist() == [2, 0, 1]
    assert pos[:3].tolist() == [[0.0, 7.0, 2.0, 14.0], [1023.0, 7.0, 2.0, 4.0], [0.0, 1030.0, 2.0, 9.0]]
    assert feat8[:3, :5].tolist() == [feat[2].tolist(), feat[0].tolist(), feat[1].tolist()]
    assert feat8[:3, 5].view(np.int32).tolist() == [2, 0, 1] and not feat8[:3, 6:].any()
    # one live run: centre of its box, farthest corner at sqrt(2) * 511.5
    assert seg[0, :3].tolist() == [511.5, 518.5, 2.0]
    assert seg[0, 3] == F32(np.sqrt(2.0 * 511.5 ** 2) * 1.00001 + 1e-6)
    # padding along y from the box centre: row 3 + k at y = 518.5 + 1e4 + 16 k
    assert pos[3, :3].tolist() == [511.5, 10518.5, 2.0] and pos[255, :3].tolist() == [511.5, 10518.5 + 16.0 * 252, 2.0]
    assert np.all(_bits(pos[3:, 3]) == 0x7FC00000) and np.all(_bits(feat8[3:, :5]) == 0x7FC00000)
    assert np.all(feat8[3:, 5].view(np.int32) == -1) and not feat8[3:, 6:].any()
    # runs 1 .. 3 hold only padding: rows 64, 128, 192 are padding rows 61, 125, 189
    for g, k in ((1, 61), (2, 125), (3, 189)):
        assert seg[g].tolist() == [511.5, 10518.5 + 16.0 * k + 512.0, 2.0, 544.0]
    assert ref.layout(xyz, feat, False, 0)[1][3, :3].tolist() == [10511.5, 518.5, 2.0]


def test_sixty_five_points_by_hand():
    """n = 65 on the x axis at 0, 1, ..., 64 handed over backwards: the order turns them round, the first
    run is 0 ... 63 (centre 31.5, radius 31.5 inflated), the second holds the one point 64: radius 1e-6."""
    xyz = np.zeros((65, 3), F32)
    xyz[:, 0] = np.arange(64, -1, -1)
    feat = np.zeros((65, 5), F32)
    feat[:, 4] = np.arange(65)
    rows, pos, feat8, seg, bbox, order = ref.layout(xyz, feat, False, 0)
    # inv = 1023 / 64 in float32 is exact; the cell of x is floor(x * 1023 / 64): strictly increasing in x
    assert order.tolist() == list(range(64, -1, -1))
    assert pos[:65, 0].tolist() == list(range(65)) and pos[:65, 3].tolist() == list(range(64, -1, -1))
    assert rows == 256 and seg.shape == (4, 4)
    assert seg[0].tolist() == [31.5, 0.0, 0.0, float(F32(31.5 * 1.00001 + 1e-6))]
    assert seg[1].tolist() == [64.0, 0.0, 0.0, float(F32(1e-6))]
    assert pos[65, :3].tolist() == [32.0 + 1.0e4, 0.0, 0.0] and pos[128, :3].tolist() == [32.0 + 1.0e4 + 16.0 * 63, 0.0, 0.0]
    assert seg[2].tolist() == [32.0 + 1.0e4 + 16.0 * 63 + 512.0, 0.0, 0.0, 544.0]
    assert seg[3].tolist() == [32.0 + 1.0e4 + 16.0 * 127 + 512.0, 0.0, 0.0, 544.0]


@pytest.mark.parametrize("flat", [(2,), (1, 2), (0, 1, 2), (0,), (0, 2)])
def test_axes_of_zero_extent_give_no_key_bits(flat):
    rng = np.random.default_rng(11)
    xyz = rng.uniform(-2.0, 2.0, (500, 3)).astype(F32)
    for a in flat:
        xyz[:, a] = F32(0.7)
    lo, hi = ref.bounding_box(xyz)
    keys = ref.morton_keys(xyz, lo, hi)
    for a in range(3):
        mask = np.uint32(0o1111111111 << a)
        if a in flat:
            assert not (keys & mask).any()
        else:
            assert (keys & mask).any()
    if len(flat) == 3:
        assert ref.layout(xyz, np.zeros((500, 5), F32), False, 0)[5].tolist() == list(range(500))


def test_extents_at_the_ends_of_float32():
    """1e-30: 1023 / ext is finite and the cells spread over 0 ... 1023; above 3.4e38 the extent is
    infinite in float32 and the axis gives cell 0 everywhere (inf * 0 is NaN, and NaN is not >= 0)."""
    x = np.zeros((5, 3), F32)
    x[:, 1] = [0.0, 1e-30, 0.5e-30, 0.25e-30, 1e-30]
    q = ref.quantise(x, *ref.bounding_box(x))
    assert q[:, 1].tolist() == [0, 1023, 511, 255, 1023] and not q[:, (0, 2)].any()
    x[:, 1] = [-3e38, 3e38, 1e38, -1e38, 3e38]
    assert not ref.quantise(x, *ref.bounding_box(x)).any()
    x[:, 1] = [-1.6e38, 1.6e38, 0.0, 0.8e38, -0.8e38]      # 3.2e38: still finite
    assert ref.quantise(x, *ref.bounding_box(x))[:, 1].tolist() == [0, 1023, 511, 767, 255]
