"""-m gpu: cvo_hip_pose_hessian (include/cvo_hip.h) against the float64 restatement of tests/pose_hessian_ref.py on the
oracle's member set, against cvo_hip_flow, and for what it must leave alone.

Tolerances.  The member set and every float32 weight are the oracle's exactly (nnz equal, f to 1e-11); g and H are
float32 per-member terms summed in float64 against float64 terms, so they agree to ~1e-6 of the sums of the absolute
products the terms are made of (pose_hessian_ref.abs_scale) -- a plain max |.| scale fails where g nearly cancels."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_hessian_ref as ref  # noqa: E402
from pose_cases import case as _case, ctx as _ctx, pose as _pose, stream as _stream, trace_bits as _trace_bits  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-6


def _oracle(po, pmode, ell, xf, ff, xm, fm, R, T, search):
    p = po.default_params(pmode)
    y = po.transform(R, T, xm)
    rp, col, val = po.se_kernel(p, ell, xf, ff, y, fm, search=search)
    rows = np.repeat(np.arange(len(xf)), np.diff(rp))
    return ref.restate(xf, y, rows, col, val, ell)


def _check(got, want, rtol=RTOL):
    assert got.nnz == want["nnz"]
    assert abs(got.f - want["f"]) <= 1e-11 * want["f"]
    assert np.all(np.abs(got.g - want["g"]) <= rtol * want["sg"]), (got.g, want["g"])
    assert np.all(np.abs(got.H - want["H"]) <= rtol * want["sH"]), np.abs(got.H - want["H"]) / want["sH"]
    assert np.array_equal(got.H, got.H.T)


@pytest.mark.parametrize("name", ["cvo_3000", "cvo_10000", "desk", "acvo_10000", "matlab_3000"])
def test_matches_restatement_on_oracle_members(pkg, po, desk, name):
    mode, omode, (xf, ff, xm, fm), ell = _case(pkg, desk, name)
    R, T = _pose()
    c = _ctx(pkg, pkg.capi.default_params(mode), xf, ff, xm, fm)
    got = c.pose_hessian(R, T, ell)
    c.close()
    search = po.SEARCH_DENSE if mode == pkg.capi.MODE_MATLAB else po.SEARCH_GRID
    want = _oracle(po, omode, ell, xf, ff, xm, fm, R, T, search)
    assert want["nnz"] > 1000
    _check(got, want)


def test_kept_format_0(pkg, po):
    xf, ff, xm, fm = pkg.data.synthetic_pair(10000, 10000, seed=13)
    R, T = _pose()
    c = _ctx(pkg, pkg.capi.default_params(pkg.capi.MODE_CVO), xf, ff, xm, fm)
    c.set_option("kept_pack", 0)
    got = c.pose_hessian(R, T, 0.1)
    c.close()
    _check(got, _oracle(po, 0, 0.1, xf, ff, xm, fm, R, T, po.SEARCH_GRID))


def test_kept_format_2(pkg, po):
    """Clouds above 65 536 rows: 8-byte entries with the weight's exponent packed (ProcessArgs::kept_packed == 2)."""
    xf, ff, xm, fm = pkg.data.synthetic_pair(70000, 70000, seed=17)
    R, T = _pose()
    c = _ctx(pkg, pkg.capi.default_params(pkg.capi.MODE_CVO), xf, ff, xm, fm)
    got = c.pose_hessian(R, T, 0.03)
    c.close()
    want = _oracle(po, 0, 0.03, xf, ff, xm, fm, R, T, po.SEARCH_GRID)
    assert want["nnz"] > 10000
    _check(got, want)


def test_consistent_with_flow(pkg, po):
    xf, ff, xm, fm = pkg.data.synthetic_pair(10000, 10000, seed=23)
    R, T = _pose()
    p = pkg.capi.default_params(pkg.capi.MODE_CVO)
    c = _ctx(pkg, p, xf, ff, xm, fm)
    ell = 0.1
    c.transform_pcd(R, T)
    out = c.flow(ell)
    h = c.pose_hessian(R, T, ell)
    c.close()
    assert h.nnz == int(out[8])
    assert abs(h.f - out[6]) <= 1e-12 * out[6]
    # the flow's own float32 terms (a / c) (x cross y): their absolute products set the scale
    y = po.transform(R, T, xm)
    rp, col, val = po.se_kernel(po.default_params(0), ell, xf, ff, y, fm, search=po.SEARCH_GRID)
    X, Y, a = xf[np.repeat(np.arange(len(xf)), np.diff(rp))].astype(np.float64), y[col].astype(np.float64), val.astype(np.float64)
    ax, ay = np.abs(X), np.abs(Y)
    cr = np.stack([ax[:, 1] * ay[:, 2] + ax[:, 2] * ay[:, 1], ax[:, 2] * ay[:, 0] + ax[:, 0] * ay[:, 2],
                   ax[:, 0] * ay[:, 1] + ax[:, 1] * ay[:, 0]], 1)
    s_om = (a[:, None] * cr).sum(0) / p.c
    s_v = (a[:, None] * np.abs(Y - X)).sum(0) / p.d
    assert np.all(np.abs(h.g[:3] * ell * ell / p.c - out[0:3]) <= RTOL * s_om)
    assert np.all(np.abs(h.g[3:] * ell * ell / p.d - out[3:6]) <= RTOL * s_v)


def test_repeated_calls_are_bit_identical(pkg):
    xf, ff, xm, fm = pkg.data.synthetic_pair(10000, 10000, seed=29)
    R, T = _pose()
    c = _ctx(pkg, pkg.capi.default_params(pkg.capi.MODE_CVO), xf, ff, xm, fm)
    a = bytes(c.pose_hessian_raw(R, T, 0.1))
    b = bytes(c.pose_hessian_raw(R, T, 0.1))
    c.close()
    assert a == b


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_no_side_effects_on_align(pkg, mode_name):
    capi = pkg.capi
    mode = capi.MODE_ACVO if mode_name == "acvo" else capi.MODE_CVO
    xf, ff, xm, fm = pkg.data.synthetic_pair(3000, 3000, seed=31, acvo=mode_name == "acvo")
    R, T = _pose()
    runs = []
    for with_h in (False, True):
        c = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
        if with_h:
            c.pose_hessian(R, T, 0.1)
        st = capi.init_state(c.params)
        n, tr = c.align(st, trace_cap=2000)
        runs.append((n, _trace_bits(tr), bytes(st)))
        c.close()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_run_sequence_with_hessian_is_bit_identical(pkg, desk, mode_name):
    Reg = pkg.Acvo if mode_name == "acvo" else pkg.Cvo
    feats = pkg.data.acvo_features if mode_name == "acvo" else pkg.data.cvo_features
    frames = [(str(k), desk["xyz%d" % k], feats(desk["rgb%d" % k])) for k in range(5)]
    out = []
    for hessian in (False, True):
        reg = Reg(device=0, stream=_stream())
        poses = []
        iters = []
        for name, x, f in frames:
            first = not reg.init
            reg.run_cvo(x, f, hessian=hessian)
            if not first:
                iters.append(reg.num_iterations)
                poses.append(reg.accum_transform.tobytes())
                if hessian:
                    assert reg.hessian is not None and reg.hessian.nnz > 0
        reg.close()
        out.append((iters, poses))
    assert out[0] == out[1]


def test_shards_add_up(pkg, po):
    capi = pkg.capi
    xf, ff, xm, fm = pkg.data.synthetic_pair(3000, 3000, seed=37)
    R, T = _pose()
    ell = 0.1
    whole_c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    whole = whole_c.pose_hessian(R, T, ell)
    whole_c.close()
    parts = []
    for r in range(2):
        c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
        lo, hi = capi.shard_range(len(xf), r, 2)
        slo, shi = capi.shard_range(len(xm), r, 2)
        c.set_shard(lo, hi, slo, shi)
        parts.append(c.pose_hessian(R, T, ell))
        c.close()
    want = _oracle(po, 0, ell, xf, ff, xm, fm, R, T, po.SEARCH_GRID)
    assert parts[0].nnz > 0 and parts[1].nnz > 0
    assert parts[0].nnz + parts[1].nnz == whole.nnz
    assert abs(parts[0].f + parts[1].f - whole.f) <= 1e-12 * whole.f
    assert np.all(np.abs(parts[0].g + parts[1].g - whole.g) <= 1e-12 * want["sg"])
    assert np.all(np.abs(parts[0].H + parts[1].H - whole.H) <= 1e-12 * want["sH"])


def test_refusals_and_empty_set(pkg):
    capi = pkg.capi
    xf, ff, xm, fm = pkg.data.synthetic_pair(2000, 2000, seed=41)
    R, T = _pose()
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(capi.CvoHipError):
            c.pose_hessian(R, T, bad)
    # far apart: no member at all, zeros and OK
    c.set_moving(xm + np.float32(100.0), fm)
    h = c.pose_hessian(R, T, 0.1)
    assert h.nnz == 0 and h.f == 0.0 and not h.g.any() and not h.H.any()
    c.close()
    # an all-reduce hook attached: refused
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    c.set_allreduce(lambda buf, count, stream: 0)
    L = capi.lib()
    out = capi.PoseHessianC()
    Rf, Tf = np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(T)
    rc = L.cvo_hip_pose_hessian(c._ctx, capi.fptr(Rf), capi.fptr(Tf), np.float32(0.1), ctypes.byref(out))
    assert rc == -1
    assert b"all-reduce" in L.cvo_hip_last_error(c._ctx)
    c.close()


def test_cpp_mirror_matches_python(pkg, desk, tmp_path):
    lib = os.path.join(ROOT, "cvo-rgbd_amd", "csrc")
    exe = str(tmp_path / "cvo_hessian_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "cvo_hessian_demo.cpp"), "-L", lib, "-lcvo_hip",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    frames = [(desk["xyz%d" % k], pkg.data.cvo_features(desk["rgb%d" % k])) for k in range(2)]
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(frames)))
        for x, f in frames:
            fh.write(struct.pack("<i", len(x)))
            fh.write(np.ascontiguousarray(x, np.float32).tobytes())
            fh.write(np.ascontiguousarray(f, np.float32).tobytes())
    lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    reg = pkg.Cvo(device=0)
    reg.set_pcd(*frames[0])
    reg.set_pcd(*frames[1])
    reg.align(hessian=True)
    h = reg.hessian
    n_iter = reg.num_iterations
    reg.close()
    tok = dict((ln.split()[0], ln.split()[1:]) for ln in lines)
    assert int(tok["n_iter"][0]) == n_iter and int(tok["nnz"][0]) == h.nnz
    assert float.fromhex(tok["f"][0]) == h.f
    assert [float.fromhex(t) for t in tok["g"]] == list(h.g)
    assert [float.fromhex(t) for t in tok["H"]] == list(h.H.reshape(36))
