"""CPU: cvo_hip_pose_matches's C-ABI (export, argument checks that need no device, struct layout) and the properties of
its restatement (tests/pose_matches_ref.py) on the oracle's member sets."""
import ctypes
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_matches_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


def test_library_exports_pose_matches(pkg):
    assert os.path.exists(pkg.capi.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    assert hasattr(lib, "cvo_hip_pose_matches")
    assert "cvo_hip_pose_matches" in pkg.capi.SYMBOLS
    assert hasattr(pkg.capi.Context, "pose_matches")
    fn = lib.cvo_hip_pose_matches
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_float] + [ctypes.c_void_p] * 3
    assert fn(None, None, None, 0.1, None, None, None) == -1   # CVO_HIP_ERR_INVALID: no context


def test_struct_layouts_match_the_c_compiler(pkg, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    summary = [f for f, _ in pkg.capi.PoseMatchesC._fields_]
    side = [f for f, _ in pkg.capi.PointMatchesC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cvo_hip.h"\nint main(void)\n{\n'
                   '    printf("%zu", sizeof(cvo_hip_pose_matches_t));\n' +
                   "".join('    printf(" %%zu", offsetof(cvo_hip_pose_matches_t, %s));\n' % f for f in summary) +
                   '    printf(" %zu", sizeof(cvo_hip_point_matches));\n' +
                   "".join('    printf(" %%zu", offsetof(cvo_hip_point_matches, %s));\n' % f for f in side) +
                   '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S, P = pkg.capi.PoseMatchesC, pkg.capi.PointMatchesC
    want = [ctypes.sizeof(S)] + [getattr(S, f).offset for f in summary] + [ctypes.sizeof(P)] + [getattr(P, f).offset for f in side]
    assert got == want


def _brute(rows, cols, val, n):
    """One side by a plain loop over the members: own index `rows`, other index `cols`."""
    support, count = [[] for _ in range(n)], np.zeros(n, np.int32)
    best, best_w = np.full(n, -1, np.int32), np.zeros(n, np.float32)
    for i, j, a in zip(rows.tolist(), cols.tolist(), val.tolist()):
        support[i].append(a)
        count[i] += 1
        if best[i] < 0 or a > best_w[i] or (a == best_w[i] and j < best[i]):
            best[i], best_w[i] = j, a
    return np.array([math.fsum(s) for s in support]), count, best, best_w


def test_restatement_against_a_plain_loop(pkg, po):
    xf, ff, xm, fm = pkg.data.synthetic_pair(700, 640, seed=5)
    T = np.array([0.02, -0.01, 0.015], np.float32)
    want = ref.matches(po, 0, 0.1, xf, ff, xm, fm, I3, T)
    rows, cols, val = want["members"]
    assert len(rows) > 1000
    for side, own, other, n in (("fixed", rows, cols, len(xf)), ("moving", cols, rows, len(xm))):
        support, count, best, best_w = _brute(own, other, val, n)
        got = want[side]
        # (fewer than 2^10 weights of 24 bits within two binades: a float64 sum of them is exact in any order)
        assert np.array_equal(got[0], support)
        assert np.array_equal(got[1], count) and np.array_equal(got[2], best) and np.array_equal(got[3], best_w)


def test_sums_add_up(pkg, po):
    xf, ff, xm, fm = pkg.data.synthetic_pair(2000, 1800, seed=9)
    T = np.array([0.02, -0.01, 0.015], np.float32)
    want = ref.matches(po, 0, 0.1, xf, ff, xm, fm, I3, T)
    rows, cols, val = want["members"]
    total = math.fsum(val.astype(np.float64).tolist())
    for side in ("fixed", "moving"):
        support, count, best, best_w = want[side]
        assert abs(math.fsum(support.tolist()) - total) <= 1e-12 * total
        assert int(count.sum()) == len(rows)
        assert np.array_equal(count > 0, best >= 0) and np.array_equal(count > 0, best_w > 0)
        assert np.all(support[count == 0] == 0.0)
        assert np.all(best_w <= support.astype(np.float32) * np.float32(1.0000002))
    assert (want["fixed"][1] > 0).sum() == len(np.unique(rows)) and (want["moving"][1] > 0).sum() == len(np.unique(cols))


def test_a_cloud_against_itself(pkg, po):
    """At the identity a point's best match is the point itself (d2 = 0 and equal features: the largest weight there is;
    another point at that weight would have to coincide with it), and A is symmetric: equal arrays on both sides."""
    x, f, _, _ = pkg.data.synthetic_pair(1500, 1500, seed=11)
    want = ref.matches(po, 0, 0.1, x, f, x, f, I3, Z3)
    fx, mv = want["fixed"], want["moving"]
    has = fx[1] > 0
    assert has.sum() > 1000
    assert np.array_equal(fx[2][has], np.arange(len(x))[has])
    assert np.array_equal(fx[1], mv[1]) and np.array_equal(fx[2], mv[2]) and np.array_equal(fx[3], mv[3])
    assert np.array_equal(fx[0], mv[0])   # (exact sums of the same weights)


def test_tie_goes_to_the_smallest_index():
    rows = np.array([0, 0, 0, 1, 1])
    cols = np.array([4, 2, 3, 3, 1])
    val = np.array([0.5, 0.5, 0.25, 0.125, 0.125], np.float32)
    out = ref.from_members(rows, cols, val, 3, 5)
    assert out["fixed"][2].tolist() == [2, 1, -1] and out["fixed"][3].tolist() == [0.5, 0.125, 0.0]
    assert out["fixed"][1].tolist() == [3, 2, 0] and out["fixed"][0].tolist() == [1.25, 0.25, 0.0]
    assert out["moving"][2].tolist() == [-1, 1, 0, 0, 0] and out["moving"][1].tolist() == [0, 1, 1, 2, 1]
