"""GPU: what a hand-over leaves in device memory (csrc/cvo_cloud.hip: Morton order, packed rows, bounding
spheres of the 64-point runs, padding rows) against the numpy restatement tests/cloud_layout_ref.py, bit for
bit, through every way a cloud can arrive, at the sizes where the hand-over changes its way and on shapes
that stress its arithmetic (tests/cloud_layout_cases.py).  The reference is held to definitions and to
hand-written answers in tests/test_cloud_layout_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_layout_cases as cases  # noqa: E402
import cloud_layout_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _contained(d, what):
    """The property the pair cull rests on, on the device's own arrays in float64: every live row lies within
    its run's radius of its run's centre (a sphere that is too small drops members of A silently)."""
    n = d["points"]
    p = d["pos"][:n, :3].astype(np.float64)
    s = d["seg"].astype(np.float64)
    run = np.arange(n) // ref.SEG
    dist = np.sqrt(((p - s[run, :3]) ** 2).sum(1))
    assert np.all(dist <= s[run, 3]), what


def _check(ctx, which, want, axis, n, what):
    """Context.device_cloud(which) equals the reference with the padding along `axis` (want[axis]), by bits."""
    d = ctx.device_cloud(which)
    assert d["points"] == n, what
    _contained(d, what)
    rows, pos, feat8, seg = want[axis][:4]
    assert d["rows"] == rows and d["pos"].shape == pos.shape and d["feat"].shape == feat8.shape and d["seg"].shape == seg.shape, what
    live = (n + ref.SEG - 1) // ref.SEG
    assert np.array_equal(_bits(d["pos"][:n]), _bits(pos[:n])), what + ": live positions"
    assert np.array_equal(_bits(d["feat"][:n]), _bits(feat8[:n])), what + ": live features"
    assert np.array_equal(_bits(d["seg"][:live, :3]), _bits(seg[:live, :3])), what + ": sphere centres"
    assert np.array_equal(_bits(d["seg"][:live, 3]), _bits(seg[:live, 3])), what + ": sphere radii"
    if rows > n and np.array_equal(_bits(d["pos"]), _bits(want[1 - axis][1])):
        assert False, what + ": padding along axis %d, expected %d" % (1 - axis, axis)
    assert np.array_equal(_bits(d["pos"]), _bits(pos)), what + ": padding rows"
    assert np.array_equal(_bits(d["feat"]), _bits(feat8)), what + ": padding features"
    assert np.array_equal(_bits(d["seg"]), _bits(seg)), what + ": padding spheres"


def _check_pair(ctx, want_f, want_m, n, what):
    """In a context whose fixed cloud arrived first: fixed pads along x, moving along y."""
    _check(ctx, 0, want_f, 0, n, what + " fixed")
    _check(ctx, 1, want_m, 1, n, what + " moving")


@pytest.mark.parametrize("shape,n", cases.CASES)
def test_hand_over_equals_the_numpy_layout(pkg, shape, n):
    """One pair of clouds of `shape` and n points through cvo_hip_set_fixed / _set_moving (one launch up to 16384
    points), the same with the option one_launch_hand_over off (rocPRIM's sort), cvo_hip_set_pcd_many into three
    contexts (row- and column-major features), the _device entry points from torch tensors, the fixed cloud after
    cvo_hip_swap_moving_to_fixed, and a context that held 4 n points before: rows, points, pos, feat and seg equal
    tests/cloud_layout_ref.py by bits, padding along x for the first cloud of a fresh context and along y for the
    second, and every live row lies inside its run's sphere in float64.
    (Radius bits rest on the device's float64 sqrt being correctly rounded.)"""
    import torch
    capi = pkg.capi
    xf, ff = cases.cloud(pkg.data, shape, n, 0)
    xm, fm = cases.cloud(pkg.data, shape, n, 1)
    want_f = [ref.layout(xf, ff, False, axis) for axis in (0, 1)]
    want_m = [ref.layout(xm, fm, False, axis) for axis in (0, 1)]
    # one launch (n <= 16384), then the moving cloud becomes the fixed one and a new moving cloud arrives
    c = capi.Context(mode=capi.MODE_CVO, device=0)
    assert c.get_option("one_launch_hand_over") == 1.0
    c.set_fixed(xf, ff); c.set_moving(xm, fm)
    _check_pair(c, want_f, want_m, n, "set_fixed / set_moving")
    c.swap_moving_to_fixed()
    _check(c, 0, want_m, 1, n, "fixed after the swap")
    assert c.device_cloud(1)["points"] == 0
    c.set_moving(xf, ff)   # (the two clouds of a context never share an axis: the newcomer takes x)
    _check(c, 1, want_f, 0, n, "moving handed over after the swap")
    _check(c, 0, want_m, 1, n, "fixed after the swap and a hand-over")
    c.close()

    # the launches of the first version (rocPRIM's radix sort), whatever the size
    c = capi.Context(mode=capi.MODE_CVO, device=0)
    c.set_option("one_launch_hand_over", 0)
    c.set_fixed(xf, ff); c.set_moving(xm, fm)
    _check_pair(c, want_f, want_m, n, "multi-launch")
    c.close()

    # a batch of three
    for col in (False, True):
        cs = [capi.Context(mode=capi.MODE_CVO, device=0) for _ in range(3)]
        conv = (lambda a: np.ascontiguousarray(a.T)) if col else (lambda a: a)
        capi.set_pcd_many(cs, [(xf, conv(ff))] * 3, [(xm, conv(fm))] * 3, layout=capi.FEAT_COLMAJOR if col else capi.FEAT_ROWMAJOR)
        for k, c in enumerate(cs):
            _check_pair(c, want_f, want_m, n, "set_pcd_many[%d] %s" % (k, "colmajor" if col else "rowmajor"))
            c.close()

    # clouds that are in device memory already
    dev = [torch.from_numpy(a).cuda() for a in (xf, ff, xm, fm)]
    torch.cuda.synchronize()
    c = capi.Context(mode=capi.MODE_CVO, device=0)
    c.set_fixed_device(dev[0].data_ptr(), dev[1].data_ptr(), n)
    c.set_moving_device(dev[2].data_ptr(), dev[3].data_ptr(), n)
    _check_pair(c, want_f, want_m, n, "device arrays")
    c.close()

    # rows shrink: a context that held 4 n points takes n; nothing of the old clouds is left inside `rows`
    xb = np.concatenate([xm, xf + np.float32(0.5), xf, xm - np.float32(0.25)])
    fb = np.concatenate([fm, ff, fm, ff])
    c = capi.Context(mode=capi.MODE_CVO, device=0)
    c.set_fixed(xb, fb); c.set_moving(xb[::-1].copy(), fb)
    assert c.device_cloud(0)["points"] == 4 * n and c.device_cloud(1)["points"] == 4 * n
    c.set_fixed(xf, ff); c.set_moving(xm, fm)
    _check_pair(c, want_f, want_m, n, "after a cloud four times the size")
    c.close()
