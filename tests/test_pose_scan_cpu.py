"""CPU: cvo_hip_pose_scan's C-ABI (export, struct layouts, the refusal that needs no device), registration.pose_grid,
the tie rule of ``best``, and -- on the oracle alone -- the scenario that motivates the scan: a pair displaced beyond
the kernel's reach, which align() leaves at the identity and which the best of a coarse grid of candidate poses
brings home.  The numbers asserted here are the ones tests/test_gpu_pose_scan.py then asks of the library."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_scan_ref as sref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib(pkg):
    assert os.path.exists(pkg.capi.LIB_PATH), "run __graft_entry__.build() first"
    return ctypes.CDLL(pkg.capi.LIB_PATH)


def test_library_exports_pose_scan(pkg):
    assert hasattr(_lib(pkg), "cvo_hip_pose_scan")
    assert "cvo_hip_pose_scan" in pkg.capi.SYMBOLS


def test_null_context_is_refused(pkg):
    f = _lib(pkg).cvo_hip_pose_scan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    assert f(None, None, None, 0, 0.1, None, None) == -1   # CVO_HIP_ERR_INVALID
    R, T = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_float * 3)()
    out, summary = pkg.capi.PoseScanEntryC(), pkg.capi.PoseScanC()
    assert f(None, R, T, 1, 0.1, ctypes.byref(out), ctypes.byref(summary)) == -1


def test_struct_layouts_match_the_c_compiler(pkg, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    entry = ("inner", "cos_angle", "mean_d2", "nnz")
    summ = ("self_fixed", "self_moving", "nnz_fixed", "nnz_moving", "count", "best", "n_fixed", "n_moving", "ell", "pad_")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cvo_hip.h"\nint main(void)\n{\n'
                   '    printf("%zu", sizeof(cvo_hip_pose_scan_entry));\n' +
                   "".join('    printf(" %%zu", offsetof(cvo_hip_pose_scan_entry, %s));\n' % f for f in entry) +
                   '    printf(" %zu", sizeof(cvo_hip_pose_scan_t));\n' +
                   "".join('    printf(" %%zu", offsetof(cvo_hip_pose_scan_t, %s));\n' % f for f in summ) +
                   '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    E, S = pkg.capi.PoseScanEntryC, pkg.capi.PoseScanC
    assert got == [ctypes.sizeof(E)] + [getattr(E, f).offset for f in entry] + \
        [ctypes.sizeof(S)] + [getattr(S, f).offset for f in summ]
    assert ctypes.sizeof(E) == 32 == pkg.capi.POSE_SCAN_ENTRY.itemsize


def test_pose_grid_order_dtype_and_shapes(pkg):
    R0 = sref.rot([0.1, 0.9, -0.2], 0.3)
    T0 = np.array([0.5, -0.25, 2.0])
    rots = [sref.rot_y(a) for a in (-10.0, 0.0, 10.0)]
    trs = [(0.0, 0.0, 0.0), (0.1, 0.0, 0.0), (0.0, 0.2, 0.0), (0.0, 0.0, -0.3)]
    Rs, Ts = pkg.registration.pose_grid(R0, T0, rots, trs)
    assert Rs.dtype == np.float32 and Ts.dtype == np.float32
    assert Rs.shape == (12, 3, 3) and Ts.shape == (12, 3)
    for i, dR in enumerate(rots):          # rotations outer ...
        for j, dT in enumerate(trs):       # ... translations inner
            assert np.array_equal(Rs[4 * i + j], (R0 @ dR).astype(np.float32))
            assert np.array_equal(Ts[4 * i + j], (T0 + np.asarray(dT)).astype(np.float32))


def test_best_takes_the_first_of_equal_poses(pkg, po):
    xf, ff, xm, fm = pkg.data.synthetic_pair(1500, 1500, seed=3)
    I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    far = np.array([40.0, 0.0, 0.0], np.float32)
    near = np.array([0.02, 0.0, 0.0], np.float32)
    s = sref.scan(po, po.MODE_CVO, 0.1, xf, ff, xm, fm, [I3, I3, I3, I3, I3], [far, near, z3, z3, far])
    assert s["nnz"][0] == 0 == s["nnz"][4] and s["inner"][2] == s["inner"][3] > s["inner"][1] > 0
    assert s["best"] == 2
    assert sref.best_of([0.0, 0.0], [0, 0]) == -1 and sref.best_of([], []) == -1


@pytest.mark.parametrize("sc", sref.SCENARIOS, ids=lambda sc: "seed%d" % sc["seed"])
def test_displaced_pair_needs_the_scan(pkg, po, sc):
    xf, ff, xm, fm = sref.scenario_clouds(pkg, sc)
    p = po.default_params(po.MODE_CVO)
    ell = sref.SCENARIO_ELL
    # from the identity: nothing within reach, one iteration, the identity comes back
    s0 = po.init_state(p)
    n0, tr0 = po.align(p, s0, xf, ff, xm, fm)
    assert n0 == 1 and tr0[0]["nnz"] == 0
    at_id = sref.scan(po, po.MODE_CVO, ell, xf, ff, xm, fm, [np.array(s0.R, np.float32).reshape(3, 3)], [np.array(s0.T, np.float32)])
    assert at_id["cos_angle"][0] == 0.0 and at_id["best"] == -1
    # the grid
    Rs, Ts = sref.scenario_grid()
    assert len(Rs) == 343
    g = sref.scan(po, po.MODE_CVO, ell, xf, ff, xm, fm, Rs, Ts)
    assert int(np.sum(g["nnz"] == 0)) == sc["empty"]
    assert g["best"] == sc["winner"]
    cs = np.sort(g["cos_angle"])
    assert abs(cs[-1] - sc["cos"]) < 5e-4 and abs(cs[-2] - sc["second"]) < 5e-4
    assert g["cos_angle"][g["best"]] == cs[-1]
    # from the winner
    s1 = po.init_state(p)
    s1.R[:] = [float(v) for v in Rs[g["best"]].ravel()]
    s1.T[:] = [float(v) for v in Ts[g["best"]]]
    n1, _ = po.align(p, s1, xf, ff, xm, fm)
    assert n1 == sc["iters"]
    fin = sref.scan(po, po.MODE_CVO, ell, xf, ff, xm, fm, [np.array(s1.R, np.float32).reshape(3, 3)], [np.array(s1.T, np.float32)])
    assert abs(fin["cos_angle"][0] - sc["final"]) < 5e-4
