"""CPU: cvo_hip_pose_hessian's C-ABI (export, argument checks, struct layout) and the closed form of the pose Hessian
(tests/pose_hessian_ref.py) against central finite differences of the frozen-set objective."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_hessian_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_pose_hessian_and_refuses_null(pkg):
    assert os.path.exists(pkg.capi.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    fn = lib.cvo_hip_pose_hessian
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    assert fn(None, None, None, 0.1, None) == -1   # CVO_HIP_ERR_INVALID
    assert "cvo_hip_pose_hessian" in pkg.capi.SYMBOLS


def test_struct_layout_matches_the_c_compiler(pkg, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "cvo_hip.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cvo_hip_pose_hessian_t), offsetof(struct cvo_hip_pose_hessian, f),
           offsetof(struct cvo_hip_pose_hessian, g), offsetof(struct cvo_hip_pose_hessian, H),
           offsetof(struct cvo_hip_pose_hessian, nnz), offsetof(struct cvo_hip_pose_hessian, ell),
           offsetof(struct cvo_hip_pose_hessian, pad_));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = pkg.capi.PoseHessianC
    want = [ctypes.sizeof(S)] + [getattr(S, f).offset for f in ("f", "g", "H", "nnz", "ell", "pad_")]
    assert got == want


def test_twist_order_is_exp_se3s(pkg):
    """exp(xi^) with xi = (omega, v) is what cvo_hip_exp_se3(omega, v, 1) returns (host maths: no GPU involved)."""
    from scipy.linalg import expm
    omega, v = np.array([0.02, -0.015, 0.03]), np.array([0.01, 0.02, -0.005])
    dR, dT = pkg.capi.exp_se3(omega.astype(np.float32), v.astype(np.float32), 1.0)
    X = np.zeros((4, 4))
    X[:3, :3] = ref.skew(omega[None])[0]
    X[:3, 3] = v
    E = expm(X)
    assert np.allclose(np.asarray(dR, np.float64).reshape(3, 3), E[:3, :3], atol=1e-6)
    assert np.allclose(np.asarray(dT, np.float64).reshape(3), E[:3, 3], atol=1e-6)


@pytest.mark.parametrize("seed,ell", [(1, 0.1), (2, 0.05), (3, 0.3)])
def test_closed_form_matches_finite_differences(seed, ell):
    rng = np.random.default_rng(seed)
    n = 300
    x = rng.uniform(-2.0, 2.0, (n, 3)) + np.array([0.0, 0.0, 2.5])
    y = x + rng.normal(0.0, 0.7 * ell, (n, 3))
    a = rng.uniform(8e-3, 1e-2, n)
    g, H = ref.member_terms(x, y, a, ell)
    g, H = g.sum(0), H.sum(0)
    h = 2e-5 * ell
    F = lambda xi: ref.frozen_objective_delta(x, y, a, ell, xi)
    e = np.eye(6)
    g_fd = np.array([(F(h * e[k]) - F(-h * e[k])) / (2 * h) for k in range(6)])
    H_fd = np.zeros((6, 6))
    for k in range(6):
        for l in range(k, 6):
            d = (F(h * (e[k] + e[l])) - F(h * (e[k] - e[l])) - F(h * (e[l] - e[k])) + F(-h * (e[k] + e[l]))) / (4 * h * h)
            H_fd[k, l] = H_fd[l, k] = d
    assert np.allclose(H, H.T)
    assert np.abs(g - g_fd).max() <= 1e-6 * np.abs(g).max()
    assert np.abs(H - H_fd).max() <= 1e-6 * np.abs(H).max()
    # the gradient is the flow's: (1 / l^2) (sum a x cross y, sum a (y - x))
    flow = np.concatenate([np.cross(x, y), y - x], 1)
    assert np.allclose(g, (a[:, None] * flow).sum(0) / ell ** 2, rtol=1e-12, atol=0)
