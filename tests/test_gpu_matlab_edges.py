"""GPU: cvo_hip_range_filter_grid_average (csrc/cvo_prep.hip) on the edges include/cvo_hip.h documents
and on arithmetic the desk clouds never reach -- bit for bit against the numpy oracle (oracle/matlab_prep.py), the
same check as tests/test_gpu_matlab.py.  The cases are tests/matlab_prep_cases.py; what the oracle answers on
them is written down in tests/test_data.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matlab_prep_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(a, b, label):
    assert a[0].dtype == np.float32 and a[1].dtype == np.uint8, label
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, label
    assert np.array_equal(a[0].view(np.uint32), np.asarray(b[0], np.float32).view(np.uint32)), label
    assert np.array_equal(a[1], b[1]), label


def _run(pkg, group):
    from oracle import matlab_prep as mp
    for label, xyz, rgb, rmax, rmin, grid in pc.GROUPS[group]():
        with np.errstate(invalid="ignore", over="ignore"):
            want = pc.expected(mp, xyz, rgb, rmax, rmin, grid)
        _same(pkg.data.prepare_matlab_cloud(xyz, rgb, rmax, rmin, grid), want, label)


def test_non_finite_points_are_dropped_whatever_the_filter(pkg):
    """NaN, +Inf and -Inf coordinates among 500 points, range filter on and off, grid 0.05 and 0: the result is the
    oracle's on the finite points alone -- they reach neither the box nor a voxel."""
    _run(pkg, "nonfinite")


def test_range_limits_are_inclusive_in_float32(pkg):
    """Ranges of exactly max_range and min_range are kept, the float32 neighbours beyond are dropped;
    min_range > max_range keeps nothing; max_range <= 0 switches the filter off whatever min_range is."""
    _run(pkg, "range_limits")
    xyz, rgb = pc.range_points()
    kept = pkg.data.prepare_matlab_cloud(xyz, rgb, pc.RANGE_MAX, pc.RANGE_MIN, 0.0)
    assert np.array_equal(kept[0], xyz[list(pc.RANGE_KEPT)])
    assert len(pkg.data.prepare_matlab_cloud(xyz, rgb, pc.RANGE_MIN, pc.RANGE_MAX, 0.0)[0]) == 0
    assert len(pkg.data.prepare_matlab_cloud(xyz, rgb, 0.0, pc.RANGE_MAX, 0.0)[0]) == len(xyz)


def test_range_is_summed_x_y_then_z(pkg):
    """32 points whose float32 range depends on the order of the sum, each with max_range = min_range = its range
    as sqrt((x*x + y*y) + z*z): the point is kept."""
    _run(pkg, "sum_order")
    xyz, r_spec, _ = pc.sum_order_points()
    for i, (label, x, c, rmax, rmin, grid) in enumerate(pc.sum_order()):
        kept = pkg.data.prepare_matlab_cloud(x, c, rmax, rmin, grid)[0]
        assert any(np.array_equal(row, xyz[i]) for row in kept), label


def test_points_on_voxel_faces(pkg):
    """origin + k * grid and the float32 neighbours on both sides, grid 1/16 (exact) and 0.05 (not), near the
    origin, at +(800, -1200, 600) and with negative coordinates."""
    _run(pkg, "voxel_faces")


def test_voxel_keys_above_32_and_53_bits(pkg):
    """A 3 m box in voxels of 1 mm and of 10 um: the upper passes of the 64-bit key sort decide the order."""
    _run(pkg, "wide_keys")


def test_a_box_of_2_to_the_63_voxels_is_refused(pkg):
    """... with CVO_HIP_ERR_INVALID and *n_out = 0, and the next call on the device is exact."""
    capi = pkg.capi
    for label, xyz, rgb, rmax, rmin, grid in pc.refused():
        with pytest.raises(capi.CvoHipError, match=r"\[-1\]"):
            pkg.data.prepare_matlab_cloud(xyz, rgb, rmax, rmin, grid)
        n = len(xyz)
        xo, co, m = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint8), C.c_int(12345)
        status = capi.lib().cvo_hip_range_filter_grid_average(
            0, xyz.ctypes.data_as(C.POINTER(C.c_float)), rgb.ctypes.data_as(C.POINTER(C.c_ubyte)), n, rmax, rmin, grid,
            xo.ctypes.data_as(C.POINTER(C.c_float)), co.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(m))
        assert status == -1 and m.value == 0, label   # CVO_HIP_ERR_INVALID
        _run(pkg, "wide_keys")


def test_heavy_voxels_and_colour_means_that_end_in_a_half(pkg):
    """70 000 points in one voxel (means 100.5, 254.5, 0.49 -> 101, 255, 0) beside 300 voxels of one point; one voxel
    for 3000 points; one point; one point kept of forty."""
    _run(pkg, "heavy_voxels")
    label, xyz, rgb, rmax, rmin, grid = pc.heavy_voxels()[0]
    out = pkg.data.prepare_matlab_cloud(xyz, rgb, rmax, rmin, grid)
    assert len(out[0]) == 301 and tuple(out[1][0]) == pc.HEAVY_COLOUR


def test_a_small_call_after_a_large_one_in_the_same_arena(pkg):
    _run(pkg, "arena")


def test_grid_size_that_is_not_positive_switches_downsampling_off(pkg):
    """grid_size 0, negative and NaN: the kept points in their order; no points in, no points out."""
    _run(pkg, "switches")
