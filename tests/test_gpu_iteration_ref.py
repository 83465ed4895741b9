"""-m gpu: the kernels behind cvo_hip_flow, cvo_hip_step_coeffs, cvo_hip_function_inner_product, one iteration of
cvo_hip_align and cvo_hip_pose_score against the float64 restatement of the reference's formulae
(tests/cvo_iteration_ref.py) -- tests/test_iteration_ref_cpu.py with the GPU in the oracle's place, through the C ABI.

The library does not hand out its member set, so the reference is evaluated over its OWN members (margin < 0) and the
count is held between the surely-in pairs and those plus the borderline ones; every borderline pair (none in these cases)
would add its whole term to the tolerance.  The tolerances are the CPU file's: K roundings of float32 times u = 2^-24
times the sum of the absolute products, derived in tests/iteration_ref_cases.py, none fitted.  The moving cloud at a pose
is the oracle's po.transform of it -- what cvo_hip_transform_pcd makes bit for bit (tests/test_gpu_parity.py), held to
R^T (y - T) in the CPU file.  Shapes: the CPU file's five and (63, 257); no launch-path switches (tests/test_gpu_paths.py).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvo_iteration_ref as ref  # noqa: E402
import iteration_ref_cases as ic  # noqa: E402
from iteration_ref_judge import Ref as _Ref, check_flow as _check_flow, check_step as _check_step  # noqa: E402

pytestmark = pytest.mark.gpu

U = ic.U
SIZES = ic.SIZES + [(63, 257)]


def _ctx(pkg, p, xf, ff, xm, fm):
    import torch
    c = pkg.capi.Context(params=p, device=0, stream=torch.cuda.current_stream().cuda_stream)
    c.set_fixed(xf, ff)
    c.set_moving(xm, fm)
    return c


def _params(pkg, mode, over=None):
    p = pkg.capi.default_params(ic.mode_id(pkg.capi, mode))
    for key, value in (over or {}).items():
        setattr(p, key, value)
    return p


@pytest.mark.parametrize("n,m", SIZES)
@pytest.mark.parametrize("mode", ["cvo", "acvo"])
def test_flow_and_step_coeffs_match_the_reference(pkg, po, mode, n, m):
    """cvo_hip_flow after cvo_hip_transform_pcd at the three poses and four length scales: out[8] between the surely-in
    count and that plus the borderline pairs, out[0:8] within the CPU file's tolerances, for acvo out[9..12] against the Axx
    and Ayy sums (Ayy over the rows i >= N alone: the reference's row rule) and counts; then cvo_hip_step_coeffs with the
    flow's own twist and omega, v ~ N(0, s), s in {0.02, 0.3, 1.0}, and cvo_hip_pick_step against numpy.roots as
    tests/test_host_math.py applies it."""
    xf, ff, xm, fm = ic.clouds(pkg, mode, n, m)
    p = _params(pkg, mode)
    c = _ctx(pkg, p, xf, ff, xm, fm)
    n_members = 0
    for ell in ic.ELLS:
        for _, R, T in ic.poses(ell):
            y = po.transform(R, T, xm)
            c.transform_pcd(R, T)
            out = c.flow(ell)
            R_ = _Ref(p, ell, xf, ff, y, fm)
            _check_flow(out, R_)
            n_members += len(R_.rows)
            if mode == "acvo":
                for k, (pa, fa, first) in ((9, (xf, ff, 0)), (11, (y, fm, n))):
                    S_ = _Ref(p, ell, pa, fa, pa, fa)
                    want, tol = S_.self_sum(first)
                    assert S_.count_ok(out[k + 1]), (k, out[k + 1], S_.sure_in)
                    assert abs(out[k] - want) <= tol, (k, out[k], want, tol)
            omega, v = out[0:3].astype(np.float32), out[3:6].astype(np.float32)
            for _, w_, v_ in [(0.0, omega, v)] + ic.twists(seed=n * 1000 + m):
                _check_step(pkg, c, R_, w_, v_, ell)
    c.close()
    assert n_members > 100 or min(n, m) == 1


@pytest.mark.parametrize("over,ells", ic.ACVO_VARIANTS)
def test_flow_where_the_other_two_cuts_decide(pkg, po, over, ells):
    """The two acvo parameter sets of iteration_ref_cases.ACVO_VARIANTS: the colour cut and the radius remove pairs of
    their own (at the shipped constants a > sp_thres implies both)."""
    xf, ff, xm, fm = ic.clouds(pkg, "acvo", 300, 260)
    p = _params(pkg, "acvo", over)
    c = _ctx(pkg, p, xf, ff, xm, fm)
    for ell in ells:
        for _, R, T in ic.poses(ell):
            c.transform_pcd(R, T)
            R_ = _Ref(p, ell, xf, ff, po.transform(R, T, xm), fm)
            _check_flow(c.flow(ell), R_)
    c.close()


@pytest.mark.parametrize("n,m", SIZES)
def test_function_inner_product_matches_the_reference(pkg, n, m):
    """cvo_hip_function_inner_product (acvo) on the clouds as set: the mean of the kept weights within (KW + 1) u of the
    reference's (no borderline pair in these cases), NaN where nothing is kept; with c_sp_thres = 0.98 as well, which
    function_inner_product's own colour cut must not follow (adaptive_cvo.cpp:392)."""
    xf, ff, xm, fm = ic.clouds(pkg, "acvo", n, m)
    for over in (None, dict(c_sp_thres=0.98)):
        p = _params(pkg, "acvo", over)
        c = _ctx(pkg, p, xf, ff, xm, fm)
        for ell in ic.ELLS:
            got = c.function_inner_product(ell)
            want, _, count, margin = ref.function_inner_product(p, ell, xf, ff, xm, fm)
            assert int(ref.classify(margin)[1].sum()) == 0
            if count == 0:
                assert np.isnan(got)
            else:
                assert abs(got - want) <= (ic.kw(p) + 1) * U * abs(want), (ell, got, want)
        c.close()


@pytest.mark.parametrize("mode", ["cvo", "acvo"])
def test_one_iteration_of_align_matches_the_reference(pkg, mode):
    """Record 0 of cvo_hip_align with max_iter = 1 from the identity pose: omega_d, v_d, sum_a and nnz against the
    reference's flow, bcde against its step terms for the record's own float32 twist, and for acvo dl against
    cvo_iteration_ref.dl on the reference's three member sets, within (KW + 10) u (S_yy + 2 S_xy + S_xx) / |den|."""
    for n, m in ((300, 260), (260, 300)):
        xf, ff, xm, fm = ic.clouds(pkg, mode, n, m)
        for ell in (0.15, 0.1, 0.06):
            p = _params(pkg, mode, dict(max_iter=1, ell_init=ell))
            c = _ctx(pkg, p, xf, ff, xm, fm)
            st = pkg.capi.init_state(p)
            n_it, tr = c.align(st, trace_cap=4)
            c.close()
            assert n_it == 1 and tr[0]["ell"] == np.float32(ell)
            t0 = tr[0]
            R_ = _Ref(p, ell, xf, ff, xm, fm)
            assert len(R_.brows) == 0 and len(R_.rows) > 100
            fl, tol = R_.flow()
            assert t0["nnz"] == len(R_.rows)
            assert np.all(np.abs(np.array(t0["omega_d"]) - fl["omega_d"]) <= tol["omega_d"])
            assert np.all(np.abs(np.array(t0["v_d"]) - fl["v_d"]) <= tol["v_d"])
            assert abs(t0["sum_a"] - fl["sum_a"]) <= tol["sum_a"]
            stp, stol = R_.step(np.array(t0["omega"], np.float32), np.array(t0["v"], np.float32))
            assert np.all(np.abs(np.array(t0["bcde"]) - stp["bcde"]) <= stol), (t0["bcde"], stp["bcde"], stol)
            if mode == "acvo":
                Sx, Sy = _Ref(p, ell, xf, ff, xf, ff), _Ref(p, ell, xm, fm, xm, fm)
                assert len(Sx.brows) == 0 and len(Sy.brows) == 0
                d = ref.dl(ell, xf, xm, (R_.rows, R_.cols, R_.am), (Sx.rows, Sx.cols, Sx.am), (Sy.rows, Sy.cols, Sy.am))
                assert (t0["nnz_xx"], t0["nnz_yy"]) == (len(Sx.rows), len(Sy.rows))
                assert abs(t0["dl"] - d["dl"]) <= ic.dl_tol(p, d), (t0["dl"], d)


def test_matlab_weight_flow_matches_the_reference(pkg, po):
    """A context with default_params(MODE_MATLAB): a = color_scale <c_i, c_j> K kept iff K >= sp_thres."""
    n_members = 0
    for n, m in ((300, 260), (63, 257)):
        xf, ff, xm, fm = ic.clouds(pkg, "matlab", n, m)
        p = _params(pkg, "matlab")
        assert p.color_scale > 0
        c = _ctx(pkg, p, xf, ff, xm, fm)
        for ell in ic.ELLS:
            for _, R, T in ic.poses(ell):
                c.transform_pcd(R, T)
                R_ = _Ref(p, ell, xf, ff, po.transform(R, T, xm), fm)
                _check_flow(c.flow(ell), R_)
                n_members += len(R_.rows)
        c.close()
    assert n_members > 1000


def test_pose_score_inner_and_count_match_the_reference(pkg, po):
    """cvo_hip_pose_score's inner and nnz at the small motion: the reference's sum_a (KW u sum a) and member count."""
    xf, ff, xm, fm = ic.clouds(pkg, "cvo", 300, 260)
    p = _params(pkg, "cvo")
    _, R, T = ic.poses(0.1)[1]
    c = _ctx(pkg, p, xf, ff, xm, fm)
    s = c.pose_score(R, T, 0.1)
    c.close()
    R_ = _Ref(p, 0.1, xf, ff, po.transform(R, T, xm), fm)
    fl, tol = R_.flow()
    assert len(R_.rows) > 100 and R_.count_ok(s.nnz)
    assert abs(s.inner - fl["sum_a"]) <= tol["sum_a"]
