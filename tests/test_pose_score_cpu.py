"""CPU: cvo_hip_pose_score's C-ABI (exports, argument checks that need no device, struct layout) and the properties of
the score's restatement (tests/pose_score_ref.py) on the oracle's member sets."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_score_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib(pkg):
    assert os.path.exists(pkg.capi.LIB_PATH), "run __graft_entry__.build() first"
    return ctypes.CDLL(pkg.capi.LIB_PATH)


def test_library_exports_pose_score(pkg):
    lib = _lib(pkg)
    for name in ("cvo_hip_pose_score", "cvo_hip_pose_score_many"):
        assert hasattr(lib, name)
        assert name in pkg.capi.SYMBOLS


def test_refusals_that_need_no_device(pkg):
    lib = _lib(pkg)
    one = lib.cvo_hip_pose_score
    one.restype = ctypes.c_int
    one.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    assert one(None, None, None, 0.1, None) == -1   # CVO_HIP_ERR_INVALID
    many = lib.cvo_hip_pose_score_many
    many.restype = ctypes.c_int
    many.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int]
    assert many(None, None, None, None, None, 0) == 0    # count 0: OK
    assert many(None, None, None, None, None, -1) == -1  # count < 0
    assert many(None, None, None, None, None, 2) == -1   # null arrays
    R, T, E = (ctypes.c_float * 18)(), (ctypes.c_float * 6)(), (ctypes.c_float * 2)(0.1, 0.1)
    out = (pkg.capi.PoseScoreC * 2)()
    ctxs = (ctypes.c_void_p * 2)(None, None)
    assert many(ctxs, R, T, E, out, 2) == -1             # null contexts


def test_struct_layout_matches_the_c_compiler(pkg, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    fields = ("inner", "self_fixed", "self_moving", "cos_angle", "mean_d2", "nnz", "nnz_fixed", "nnz_moving",
              "fixed_matched", "moving_matched", "n_fixed", "n_moving", "ell", "pad_")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cvo_hip.h"\nint main(void)\n{\n'
                   '    printf("%zu", sizeof(cvo_hip_pose_score_t));\n' +
                   "".join('    printf(" %%zu", offsetof(struct cvo_hip_pose_score, %s));\n' % f for f in fields) +
                   '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = pkg.capi.PoseScoreC
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]


def _rot(axis, th):
    ax = np.asarray(axis, np.float64)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def test_cloud_against_itself_is_one(pkg, po):
    x, f, _, _ = pkg.data.synthetic_pair(2000, 2000, seed=5)
    for mode in (po.MODE_CVO, po.MODE_ACVO):
        p = po.default_params(mode)
        rows, cols, a = ref.members(po, p, 0.1, x, f, x, f, po.SEARCH_GRID)
        assert np.array_equal(np.unique(rows[rows == cols]), np.arange(len(x)))   # the diagonal is in the self set
        s = ref.score(po, mode, 0.1, x, f, x, f, np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
        assert s["nnz"] == s["nnz_fixed"] == s["nnz_moving"]
        assert s["cos_angle"] == 1.0
        assert s["mean_d2"] >= 0.0 and s["fixed_matched"] == s["moving_matched"] == len(x)


def test_common_rigid_motion_keeps_the_cosine(pkg, po):
    xf, ff, xm, fm = pkg.data.synthetic_pair(3000, 3000, seed=7)
    I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    base = ref.score(po, po.MODE_CVO, 0.1, xf, ff, xm, fm, I3, z3)
    G = _rot([0.2, 1.0, -0.4], 0.7).astype(np.float32)
    g = np.array([0.5, -1.2, 0.3], np.float32)
    # both clouds moved by (G, g): the moving cloud is still the fixed one's neighbour at the identity
    moved = ref.score(po, po.MODE_CVO, 0.1, xf @ G.T + g, ff, xm @ G.T + g, fm, I3, z3)
    assert base["nnz"] > 1000
    assert abs(moved["cos_angle"] - base["cos_angle"]) < 1e-5


@pytest.mark.parametrize("k,cos_id,cos_conv", [(0, 0.9768, 0.9873), (1, 0.9837, 0.9942)])
def test_desk_converged_pose_scores_higher(pkg, po, desk, k, cos_id, cos_conv):
    p = po.default_params(po.MODE_CVO)
    xf, ff = desk["xyz%d" % k], pkg.data.cvo_features(desk["rgb%d" % k])
    xm, fm = desk["xyz%d" % (k + 1)], pkg.data.cvo_features(desk["rgb%d" % (k + 1)])
    s = po.init_state(p)
    po.align(p, s, xf, ff, xm, fm)
    R, T = np.array(s.R, np.float32).reshape(3, 3), np.array(s.T, np.float32)
    ell = 0.15
    at_id = ref.score(po, po.MODE_CVO, ell, xf, ff, xm, fm, np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    conv = ref.score(po, po.MODE_CVO, ell, xf, ff, xm, fm, R, T)
    assert conv["cos_angle"] > at_id["cos_angle"]
    assert abs(at_id["cos_angle"] - cos_id) < 5e-4 and abs(conv["cos_angle"] - cos_conv) < 5e-4
    assert 0.0 < conv["cos_angle"] < 1.0
    # a self cosine is exactly one
    own = ref.score(po, po.MODE_CVO, ell, xf, ff, xf, ff, np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    assert own["cos_angle"] == 1.0
