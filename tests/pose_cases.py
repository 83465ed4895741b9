"""What the -m gpu tests of the pose queries (tests/test_gpu_pose_*.py) share: the stream, the test pose, a context with
both clouds set, the named cases and how traces are compared.  A plain module; no test lives here."""
import numpy as np


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def pose():
    ax = np.array([0.3, -0.5, 0.8])
    ax /= np.linalg.norm(ax)
    th = 0.02
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    return R.astype(np.float32), np.array([0.01, -0.02, 0.015], np.float32)


def ctx(pkg, params, xf, ff, xm, fm):
    c = pkg.capi.Context(params=params, device=0, stream=stream())
    c.set_fixed(xf, ff)
    c.set_moving(xm, fm)
    return c


def case(pkg, desk, name):
    """(capi mode, oracle mode, clouds, ell) of a named case."""
    capi = pkg.capi
    if name == "desk":
        xf, ff = desk["xyz0"], pkg.data.cvo_features(desk["rgb0"])
        xm, fm = desk["xyz1"], pkg.data.cvo_features(desk["rgb1"])
        return capi.MODE_CVO, 0, (xf, ff, xm, fm), 0.1
    kind, n = name.split("_")
    n = int(n)
    clouds = pkg.data.synthetic_pair(n, n, seed=n % 97 + 3, acvo=kind == "acvo")
    return {"cvo": capi.MODE_CVO, "acvo": capi.MODE_ACVO, "matlab": capi.MODE_MATLAB}[kind], \
        {"cvo": 0, "acvo": 1, "matlab": 2}[kind], clouds, (0.15 if kind == "matlab" else 0.1)


def trace_bits(tr):
    """A trace as tests/test_gpu_paths.py compares traces bit for bit: the members and the float32 twist and step of every
    iteration (the float64 sums and the bookkeeping fields of a record depend on which launch path an iteration took --
    resident runs or not, a matter of timing -- not on the registration)."""
    return [(t["nnz"], t["step"], tuple(t["omega"]), tuple(t["v"])) for t in tr]
