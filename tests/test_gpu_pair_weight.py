"""-m gpu: the kernels' pair weight (csrc/cvo_pair.h: exp_neg, the three cuts, the float32 weight) at the parameter sets
of tests/pair_weight_cases.py, far from the shipped constants, through the C ABI.

Per pair.  On the star of isolated pairs every member is (j, j), so cvo_hip_pose_matches' count[j] is the membership of
pair j and best_w[j] its float32 weight as bits: both EQUAL the oracle's (the arithmetic contract), borderline
pairs included; the weights are also held to the float64 reference within iteration_ref_cases.weight_bound.  The sums of
cvo_hip_flow, cvo_hip_pose_score, cvo_hip_pose_hessian and cvo_hip_pose_scan follow by the rules of their own tests.
The sums, on dense pairs: cvo_hip_flow and cvo_hip_step_coeffs through tests/iteration_ref_judge.py with flow_tol / step_tol
of the set's parameters, and against the oracle by tests/test_gpu_parity.py's rule.
The loop: one registration per set against po.align, with and without resident runs, under both list plans; sixteen
registrations that mix the sets through cvo_hip_align_many.
The sets without a member (tau <= 0, tau_c <= 0): zeros and CVO_HIP_OK, and a context that is usable afterwards.

No tolerance here comes from an observed error: each is weight_bound, flow_tol, step_tol, a bound a header or an existing
test states, or bit equality.  Every test prints what it compared and its wall time (pytest -s)."""
import math
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iteration_ref_cases as ic  # noqa: E402
import pair_weight_cases as pw  # noqa: E402
import pose_matches_ref  # noqa: E402
import pose_scan_ref  # noqa: E402
import pose_score_ref  # noqa: E402
from iteration_ref_judge import Ref as _Ref, check_flow as _check_flow, check_self as _check_self, check_step as _check_step  # noqa: E402

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-11   # float64 sums of the same float32 terms in another order (tests/test_gpu_parity.py, test_gpu_pose_score.py)
WITH_MEMBERS = [s.name for s in pw.SETS if s.members]
WITHOUT = [s.name for s in pw.SETS if not s.members]
I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    print("[%s: %.2f s]" % (request.node.name, time.perf_counter() - t0))


class _Worst:
    """The largest error / tolerance per quantity (iteration_ref_judge's `worst`)."""

    def __init__(self):
        self.frac = {}

    def see(self, key, err, tol):
        with np.errstate(divide="ignore", invalid="ignore"):
            f = float(np.max(np.nan_to_num(np.asarray(err, np.float64) / np.asarray(tol, np.float64))))
        self.frac[key] = max(self.frac.get(key, 0.0), f)

    def __str__(self):
        return ", ".join("%s %.3f" % kv for kv in sorted(self.frac.items()))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _ctx(pkg, p, xf, ff, xm, fm, options=()):
    c = pkg.capi.Context(params=p, device=0, stream=_stream())
    for key, value in options:
        c.set_option(key, value)
    c.set_fixed(xf, ff)
    c.set_moving(xm, fm)
    return c


def _close(a, b, rtol=SUM_RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= rtol * max(np.abs(b).max(), 1e-300)


def _last_error(pkg, c):
    return pkg.capi.lib().cvo_hip_last_error(c._ctx).decode()


# ---- per pair, on the star
@pytest.mark.parametrize("name", WITH_MEMBERS)
def test_star_pair_by_pair(pkg, po, name):
    """For every length scale and pose of the set: count, best and best_w of both sides equal the oracle's members and
    float32 weights (the number of weights that differ is printed before it is asserted to be zero); summary.nnz and
    summary.inner are the oracle's; flow's sum_a and nnz, pose_score's inner / nnz / mean_d2, pose_hessian's f / nnz
    likewise; pose_scan over the two poses has pose_score's nnz and an inner within the header's 2 g inner,
    g = nnz u / (1 - nnz u), u = 2^-53.  The kept weights are within weight_bound of the float64 reference."""
    s = pw.BY_NAME[name]
    p = s.params(pkg.capi)
    compared = differ = 0
    worst = 0.0
    for ell in s.ells:
        for ps in pw.POSES:
            st = pw.star(po, name, ell, ps)
            K = len(st["xf"])
            rows, val, R, T = st["rows"], st["val"], st["R"], st["T"]
            tag = (name, ell, ps)
            c = _ctx(pkg, p, st["xf"], st["ff"], st["xm"], st["fm"])
            m = c.pose_matches(R, T, ell)
            sc = c.pose_score(R, T, ell)
            h = c.pose_hessian(R, T, ell)
            c.transform_pcd(R, T)
            out = c.flow(ell)
            Rs, Ts = np.stack([pw.pose(q)[0] for q in pw.POSES]), np.stack([pw.pose(q)[1] for q in pw.POSES])
            scan = c.pose_scan(Rs, Ts, ell)
            scores = [c.pose_score(Rs[k], Ts[k], ell) for k in range(len(Rs))]
            c.close()
            want = pose_matches_ref.from_members(rows, rows, val, K, K)
            for side_name in ("fixed", "moving"):
                got, w = getattr(m, side_name), want[side_name]
                bad_w = int((got.best_w.view(np.uint32) != w[3].view(np.uint32)).sum())
                bad_c = int((got.count != w[1]).sum())
                differ += bad_w
                compared += len(rows)
                if bad_w or bad_c:
                    j = np.flatnonzero((got.best_w.view(np.uint32) != w[3].view(np.uint32)) | (got.count != w[1]))[:5]
                    print(tag, side_name, "weights that differ:", bad_w, "memberships that differ:", bad_c,
                          "first:", j, got.best_w[j], w[3][j], got.count[j], w[1][j])
                assert bad_c == 0, (tag, side_name, bad_c)                       # membership, borderline pairs included
                assert bad_w == 0, (tag, side_name, bad_w)                       # the weight, by bits
                assert np.array_equal(got.best, w[2]), (tag, side_name)          # best[j] == j for a member, -1 otherwise
                assert np.array_equal(got.best[got.count > 0], np.flatnonzero(got.count > 0))
            inner = math.fsum(val.astype(np.float64).tolist())
            assert m.nnz == len(rows) and abs(m.inner - inner) <= SUM_RTOL * inner, (tag, m.nnz, len(rows), m.inner, inner)
            assert int(out[8]) == len(rows) and abs(out[6] - inner) <= SUM_RTOL * inner, tag
            d2 = pose_score_ref.sq_dist(st["xf"], st["y"], rows, rows)
            mean_d2 = float(np.sum(val.astype(np.float64) * d2)) / inner
            assert sc.nnz == len(rows) and abs(sc.inner - inner) <= SUM_RTOL * inner, tag
            assert abs(sc.mean_d2 - mean_d2) <= 1e-6 * mean_d2, (tag, sc.mean_d2, mean_d2)
            assert h.nnz == len(rows) and abs(h.f - inner) <= SUM_RTOL * inner, tag
            for k, one in enumerate(scores):
                g = pose_scan_ref.gamma(max(int(one.nnz), 1))
                assert scan.nnz[k] == one.nnz, (tag, k, scan.nnz[k], one.nnz)
                assert abs(scan.inner[k] - one.inner) <= 2 * g * one.inner, (tag, k)
            assert scan.nnz[pw.POSES.index(ps)] == len(rows)
            # the float64 reference, outside nothing: every kept weight has its bound
            bound = ic.weight_bound(st["p"], ell, st["a"][rows], st["d2"][rows], st["d2c"][rows])
            frac = float(np.max(np.abs(m.fixed.best_w[rows].astype(np.float64) - st["a"][rows]) / bound))
            assert frac <= 1.0, (tag, frac)
            worst = max(worst, frac)
            assert np.array_equal((m.fixed.count > 0) & ~st["border"], st["sure_in"]), tag
    print("%s: %d members compared pair by pair (both sides), %d weights differ from the oracle's; worst error / weight_bound "
          "against the float64 reference %.3f" % (name, compared, differ, worst))


# ---- the sums, on the dense pairs
@pytest.mark.parametrize("name", WITH_MEMBERS)
def test_dense_flow_and_step_sums(pkg, po, name):
    """cvo_hip_flow and cvo_hip_step_coeffs on (300, 260) and (257, 63) at the three poses of iteration_ref_cases.poses:
    within flow_tol / step_tol of the float64 reference over its own members, and equal to the oracle's by the rule of
    tests/test_gpu_parity.py (nnz equal, the float32 twist identical, the float64 sums to 1e-11 / 1e-10 of their largest
    component).  acvo: the Axx / Ayy sums and counts as well."""
    s = pw.BY_NAME[name]
    p, op = s.params(pkg.capi), s.params(po)
    ell = pw.dense_ell(s)
    worst = _Worst()
    members = 0
    for n, m in pw.DENSE_SIZES:
        xf, ff, xm, fm = ic.clouds(pkg, s.mode, n, m)
        c = _ctx(pkg, p, xf, ff, xm, fm)
        for ps in ic.poses(ell):
            _, R, T = ps
            d = pw.dense_case(pkg, po, name, n, m, ell, ps)
            y = d["y"]
            c.transform_pcd(R, T)
            out = c.flow(ell)
            R_ = _Ref(p, ell, xf, ff, y, fm)
            _check_flow(out, R_, worst)
            members += len(R_.rows)
            om, v, sa, sad2 = po.flow(op, ell, xf, y, d["csr"])
            assert int(out[8]) == len(d["rows"]), (name, n, m, ps[0], int(out[8]), len(d["rows"]))
            assert _close(out[0:3], om) and _close(out[3:6], v) and _close([out[6]], [sa]) and _close([out[7]], [sad2])
            omega, vv = om.astype(np.float32), v.astype(np.float32)
            assert np.array_equal(out[0:3].astype(np.float32), omega) and np.array_equal(out[3:6].astype(np.float32), vv)
            if s.mode == "acvo":
                for k, (pa, fa, first) in ((9, (xf, ff, 0)), (11, (y, fm, n))):
                    _check_self(out, k, _Ref(p, ell, pa, fa, pa, fa), first, worst)
                    rp2, _, _ = po.se_kernel(op, ell, pa, fa, pa, fa, search=po.SEARCH_GRID)
                    assert int(out[k + 1]) == int(rp2[-1]), (name, k)
            for _, w_, v_ in [(0.0, omega, vv)] + ic.twists(seed=n * 1000 + m):
                bcde, _ = _check_step(pkg, c, R_, w_, v_, ell, worst)
                assert _close(bcde, po.step_coeffs(ell, w_, v_, xf, y, d["csr"]), 1e-10), (name, n, m, ps[0])
        c.close()
    assert members > 500
    print("%s: %d members in the dense sums; worst error / tolerance: %s" % (name, members, worst))


# ---- the loop
def _oracle_align(po, s, xf, ff, xm, fm):
    op = s.params(po)
    op.max_iter = 30
    st = po.init_state(op)
    n_or, tr_or = po.align(op, st, xf, ff, xm, fm, search=pw.search_of(po, s), trace_cap=30)
    return n_or, tr_or, st


def _same_registration(pkg, po, tag, n_it, tr, st, n_or, tr_or, st_or):
    """tests/test_gpu_parity.py test_align_matches_oracle_synthetic's comparison."""
    assert n_it == n_or and len(tr) == len(tr_or), (tag, n_it, n_or)
    for k, (a, b) in enumerate(zip(tr, tr_or)):
        assert a["nnz"] == b["nnz"] and a["ell"] == b["ell"], (tag, k, a["nnz"], b["nnz"])
        assert a["omega"] == b["omega"] and a["v"] == b["v"] and a["step"] == b["step"], (tag, k)
        assert a["k"] == b["k"] and a["exit_code"] == b["exit_code"], (tag, k)
        assert abs(a["sum_a"] - b["sum_a"]) <= SUM_RTOL * max(1.0, abs(b["sum_a"])), (tag, k)
    T_gpu, T_or = np.array(st.transform, np.float32).reshape(4, 4), po.state_matrices(st_or)[0]
    rot, tra = pkg.data.rel_pose_error(T_gpu, T_or)
    assert rot <= 1e-6 and tra <= 1e-6, (tag, rot, tra)
    assert np.allclose(np.array(st.accum_transform, np.float32).reshape(4, 4), po.state_matrices(st_or)[2], rtol=0, atol=1e-7), tag
    assert st.iter == st_or.iter, tag


@pytest.mark.parametrize("name", [s.name for s in pw.SETS])
def test_one_registration_equals_the_oracles(pkg, po, name):
    """(300, 260) with max_iter 30 and trace_cap 30: the iteration count, every trace record and the final state equal
    po.align's with the same parameters -- with resident runs at their default and off, under the synchronous and the
    asynchronous list plan.  Wide radii make every pair a member; where the kept list outgrows its first capacity the
    grow-and-resume path runs ("list_grows", printed).  Measured on an MI355X: no set's list grew at this size, in any of the
    four settings (profiles/pair_weight.json); tests/test_gpu_engine_begin_end.py holds that path."""
    s = pw.BY_NAME[name]
    xf, ff, xm, fm = ic.clouds(pkg, s.mode, 300, 260)
    n_or, tr_or, st_or = _oracle_align(po, s, xf, ff, xm, fm)
    assert (tr_or[0]["nnz"] > 0) == s.members
    grows = {}
    for runs in (None, 0):
        for async_builds in (0, 1):
            p = s.params(pkg.capi)
            p.max_iter = 30
            opts = (("async_builds", async_builds),) + ((("resident_runs", runs),) if runs is not None else ())
            c = _ctx(pkg, p, xf, ff, xm, fm, opts)
            st = pkg.capi.init_state(p)
            n_it, tr = c.align(st, trace_cap=30)
            grows[(runs, async_builds)] = int(c.get_option("list_grows"))
            assert _last_error(pkg, c) == ""
            c.close()
            _same_registration(pkg, po, (name, runs, async_builds), n_it, tr, st, n_or, tr_or, st_or)
    print("%s: %d iterations, first nnz %d of %d candidates; list_grows by (resident_runs, async_builds): %s"
          % (name, n_or, tr_or[0]["nnz"], 300 * 260, grows))


def test_sixteen_mixed_registrations_through_align_many(pkg, po):
    """Sixteen contexts, each with a fusable set's parameters (all but the MATLAB weight, which stays out of the engines
    by design) and a pair of its own, through cvo_hip_align_many: each equals its own cvo_hip_align (the rule of
    tests/test_gpu_engine_begin_end.py: the iteration count and the bytes of the final state), and "engine_begins" says
    the cvo registrations -- thirteen, a group the engines take -- went through the engines (the three acvo ones are a
    group the call leaves to their own streams)."""
    import torch
    capi = pkg.capi
    fus = [s for s in pw.SETS if s.fusable]
    sets = [fus[b % len(fus)] for b in range(16)]
    n_cvo = sum(s.mode == "cvo" for s in sets)
    assert len(fus) == 12 and n_cvo > 12   # (more than twelve of a mode: the call does not leave them to their own streams)
    ctxs, streams = [], []
    for b, s in enumerate(sets):
        n = 300 + 7 * b
        xf, ff, xm, fm = pkg.data.synthetic_pair(n, n - 40, seed=pkg.data.SEED_CFG5_BASE + 300 + b, acvo=s.mode == "acvo")
        p = s.params(capi)
        p.max_iter = 30
        stream = torch.cuda.Stream()
        c = capi.Context(params=p, device=0, stream=stream.cuda_stream, graph_capture=True)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        ctxs.append(c); streams.append(stream)
    keys = ("engine_begins", "list_grows")
    try:
        before = {k: sum(int(c.get_option(k)) for c in ctxs) for k in keys}
        for _ in range(2):   # (the second call re-uses the engines' tables and captured batches)
            states = [capi.init_state(c.params) for c in ctxs]
            its = capi.align_many(ctxs, states)
        moved = {k: sum(int(c.get_option(k)) for c in ctxs) - before[k] for k in keys}
        grew = [sets[b].name for b, c in enumerate(ctxs) if int(c.get_option("list_grows")) > 0]
        print("iterations", list(its), "counters", moved, "sets whose lists grew:", grew)
        for b, c in enumerate(ctxs):
            st = capi.init_state(c.params)
            n_l, _ = c.align(st, trace_cap=0)
            assert n_l == its[b], (b, sets[b].name, n_l, its[b])
            assert bytes(st) == bytes(states[b]), (b, sets[b].name)
            assert (its[b] == 1) or sets[b].members, (b, sets[b].name, its[b])
        assert moved["engine_begins"] >= 2 * n_cvo, moved
    finally:
        for c in ctxs:
            c.close()


# ---- the sets without a member
@pytest.mark.parametrize("name", WITHOUT)
def test_no_member_sets_return_zeros_and_leave_the_context_usable(pkg, po, name):
    """tau <= 0 (sp_thres >= sigma^2) or tau_c <= 0 (c_sp_thres >= c_sigma^2): flow, pose_score, pose_matches, pose_scan
    and pose_hessian return zeros and CVO_HIP_OK on the star and on a dense pair, align returns the oracle's iteration
    count and state, cvo_hip_last_error stays empty, and after set_params back to the shipped constants a registration on
    the same context equals a fresh context's."""
    capi = pkg.capi
    s = pw.BY_NAME[name]
    p = s.params(capi)
    ell = s.ells[0]
    st_ = pw.star(po, name, ell, "small")
    assert len(st_["rows"]) == 0
    dense = ic.clouds(pkg, s.mode, 300, 260)
    for xf, ff, xm, fm, R, T in ((st_["xf"], st_["ff"], st_["xm"], st_["fm"], st_["R"], st_["T"]), dense + (I3, Z3)):
        c = _ctx(pkg, p, xf, ff, xm, fm)
        c.transform_pcd(R, T)
        out = c.flow(ell)
        assert not out[0:9].any(), out
        sc = c.pose_score(R, T, ell)
        assert (sc.nnz, sc.inner, sc.cos_angle, sc.mean_d2, sc.fixed_matched, sc.moving_matched) == (0, 0.0, 0.0, 0.0, 0, 0)
        assert (sc.nnz_fixed, sc.nnz_moving, sc.self_fixed, sc.self_moving) == (0, 0, 0.0, 0.0)
        m = c.pose_matches(R, T, ell)
        assert (m.nnz, m.inner, m.fixed_matched, m.moving_matched) == (0, 0.0, 0, 0)
        for side in (m.fixed, m.moving):
            assert not side.support.any() and not side.count.any() and not side.best_w.any() and np.all(side.best == -1)
        scan = c.pose_scan(np.stack([I3, R]), np.stack([Z3, T]), ell)
        assert scan.best == -1 and not scan.nnz.any() and not scan.inner.any() and not scan.mean_d2.any() and not scan.cos_angle.any()
        h = c.pose_hessian(R, T, ell)
        assert h.nnz == 0 and h.f == 0.0 and not h.g.any() and not h.H.any()
        assert _last_error(pkg, c) == ""
        c.close()
    # the loop
    xf, ff, xm, fm = dense
    n_or, tr_or, st_or = _oracle_align(po, s, xf, ff, xm, fm)
    assert n_or == 1 and tr_or[0]["exit_code"] == 1 and tr_or[0]["nnz"] == 0
    p.max_iter = 30
    c = _ctx(pkg, p, xf, ff, xm, fm)
    st = capi.init_state(p)
    n_it, tr = c.align(st, trace_cap=30)
    _same_registration(pkg, po, name, n_it, tr, st, n_or, tr_or, st_or)
    assert tr[0]["step"] == np.float32(p.min_step)
    assert np.array_equal(np.array(st.transform, np.float32).reshape(4, 4), np.eye(4, dtype=np.float32))
    assert _last_error(pkg, c) == ""
    # back to the shipped constants on the same context: what a fresh context computes
    shipped = capi.default_params(ic.mode_id(capi, s.mode))
    shipped.max_iter = 30
    c.set_params(shipped)
    st1 = capi.init_state(shipped)
    n1, tr1 = c.align(st1, trace_cap=30)
    sc1 = c.pose_score(I3, Z3, ell)
    c.close()
    f = _ctx(pkg, shipped, xf, ff, xm, fm)
    st2 = capi.init_state(shipped)
    n2, tr2 = f.align(st2, trace_cap=30)
    sc2 = f.pose_score(I3, Z3, ell)
    f.close()
    assert n1 == n2 and n1 > 1 and tr1[0]["nnz"] > 0
    assert [(t["nnz"], t["step"], tuple(t["omega"]), tuple(t["v"])) for t in tr1] == [(t["nnz"], t["step"], tuple(t["omega"]), tuple(t["v"])) for t in tr2]
    assert bytes(st1) == bytes(st2) and tuple(sc1) == tuple(sc2)
