"""-m gpu: the library on the hostile geometry of tests/hostile_cases.py -- clouds far from the origin, a blob, duplicates,
zero extent, very unequal and tiny sizes, sizes around the run / tile / block boundaries, a jump -- against the CPU oracle.

The bounds the library skips work by (the MFMA pre-filter's slack, the bounding-sphere cull of the Morton runs, the travel
bounds of the lists and records) are meant to be conservative: the exact per-pair test decides membership in A.  A bound a
little too tight loses a member silently -- a few 1e-5 of a sum -- so everything here counts members EXACTLY, per row where
it can, at poses that rotate about the fixed cloud's box centre by 0 .. 0.02 rad.

Why the primitives and the extremal stream, and not registrations alone: from the identity the far* cases end after 1 - 7
iterations by the algorithm's own float32 break tests (the step of a cloud 1.5 km away rounds to nothing), so a registration
there says almost nothing about the culling.

Tolerances are those of the tests the fields come from: tests/test_gpu_parity.py (flow, step, align), test_gpu_pose_score.py,
_hessian.py, _matches.py and _scan.py (the pose queries)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_cases as hc  # noqa: E402
import pose_hessian_ref as href  # noqa: E402
import pose_matches_ref as mref  # noqa: E402
import pose_scan_ref as sref  # noqa: E402
import pose_score_ref as ref  # noqa: E402
from pose_cases import ctx as _ctx, stream as _stream  # noqa: E402

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-11   # tests/test_gpu_parity.py
HESS_RTOL = 1e-6   # tests/test_gpu_pose_hessian.py
HESS_ELL = 0.06    # the Hessian's restatement holds 36 float64 per member: one length scale, every pose
MODES = ("cvo", "acvo")


def _modes(pkg, po, mode_name):
    acvo = mode_name == "acvo"
    return acvo, (pkg.capi.MODE_ACVO if acvo else pkg.capi.MODE_CVO), (po.MODE_ACVO if acvo else po.MODE_CVO)


def _close(a, b, rtol=SUM_RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), 1e-300)
    return np.abs(a - b).max() <= rtol * scale


def _self_sum(X, csr, first, ell):
    """sum over the rows >= first of a self set of inv_l3 a d2, as tests/test_gpu_parity.py test_acvo_self_terms_match_oracle."""
    inv_l3 = np.float32(1) / (np.float32(ell) * np.float32(ell) * np.float32(ell))
    rp, col, val = csr
    rows = np.repeat(np.arange(X.shape[0]), np.diff(rp))
    keep = rows >= first
    e = (X[rows[keep]] - X[col[keep]]).astype(np.float32)
    d2 = np.float32(0) + e[:, 0] * e[:, 0]
    d2 = (e[:, 1].astype(np.float64) * e[:, 1] + d2).astype(np.float32)   # fma
    d2 = (e[:, 2].astype(np.float64) * e[:, 2] + d2).astype(np.float32)
    return float((((inv_l3 * val[keep]).astype(np.float32) * d2).astype(np.float32)).astype(np.float64).sum())


def _all_pairs_d2(x, y):
    """Float64 squared distances of all pairs of the float32 coordinates."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d2 = np.zeros((len(x), len(y)))
    for a in range(3):
        e = x[:, a][:, None] - y[:, a][None, :]
        d2 += e * e
    return d2


def _check_matches(m, want, tag):
    """tests/test_gpu_pose_matches.py _check_against: count, best, best_w equal; support = fsum of the point's weights."""
    rows, cols, val = want["members"]
    assert m.exact, tag
    assert m.nnz == len(rows), (tag, m.nnz, len(rows))
    for side, own in (("fixed", rows), ("moving", cols)):
        got, w = getattr(m, side), want[side]
        n = len(w[0])
        for k, what in ((1, "count"), (2, "best"), (3, "best_w")):
            bad = np.flatnonzero(got[k] != w[k])
            assert len(bad) == 0, (tag, side, what, bad[:5], got[k][bad[:5]], w[k][bad[:5]])
        order = np.argsort(own, kind="stable")
        cuts = np.searchsorted(np.asarray(own)[order], np.arange(n + 1))
        v = val.astype(np.float64)[order].tolist()
        exact = np.array([math.fsum(v[cuts[k]:cuts[k + 1]]) for k in range(n)])
        assert np.array_equal(got.support, exact), (tag, side)
        assert np.all(np.abs(got.support - w[0]) <= 1e-10 * w[0]), (tag, side)
    for side, matched in ((m.fixed, m.fixed_matched), (m.moving, m.moving_matched)):
        assert int(side.count.astype(np.int64).sum()) == m.nnz, tag
        assert int((side.count > 0).sum()) == matched, tag
        assert abs(math.fsum(side.support.tolist()) - m.inner) <= 1e-11 * m.inner, tag
        if m.nnz == 0:   # an empty A: zeros, and no best
            assert not side.support.any() and not side.count.any() and not side.best_w.any() and np.all(side.best == -1), tag


def _check_score(got, want, tag):
    """tests/test_gpu_pose_score.py _check."""
    for k in ("nnz", "nnz_fixed", "nnz_moving", "fixed_matched", "moving_matched"):
        assert getattr(got, k) == want[k], (tag, k, getattr(got, k), want[k])
    for k in ("inner", "self_fixed", "self_moving"):
        assert abs(getattr(got, k) - want[k]) <= 1e-11 * want[k], (tag, k, getattr(got, k), want[k])
    assert abs(got.mean_d2 - want["mean_d2"]) <= 1e-6 * want["mean_d2"], (tag, got.mean_d2, want["mean_d2"])
    assert abs(got.cos_angle - want["cos_angle"]) <= 1e-10, tag
    if want["nnz"] == 0:
        assert got.inner == 0.0 and got.mean_d2 == 0.0 and got.cos_angle == 0.0, tag


# ---------------------------------------------------------------------------
# 3 + 5b: the primitives and the pose queries at every case x pose, one length scale per test
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ell", hc.ELLS)
@pytest.mark.parametrize("mode_name", MODES)
@pytest.mark.parametrize("name", hc.NAMES)
def test_primitives_and_pose_queries(pkg, po, name, mode_name, ell):
    """At every pose of hostile_cases.poses: cvo_hip_flow and cvo_hip_step_coeffs against the oracle on its own transformed
    cloud (counts exact, float64 sums at SUM_RTOL, float32 twist identical, B..E at 1e-10, the same step; acvo: the self sets
    with the Ayy row rule), cvo_hip_pose_matches per row and per column (a lost member names its row), the counts against
    float64 all-pairs distances that pass through no search at all, and cvo_hip_pose_score / _hessian against their
    restatements and each other."""
    acvo, mode, omode = _modes(pkg, po, mode_name)
    capi = pkg.capi
    xf, ff, xm, fm = hc.clouds(pkg.data, name, acvo)
    n, m = len(xf), len(xm)
    p = po.default_params(omode)
    tau = po.thresholds(p, ell)[0]
    c = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
    Axx = po.se_kernel(p, ell, xf, ff, xf, ff, search=po.SEARCH_GRID)
    sf = float(np.sum(Axx[2].astype(np.float64)))
    Amm = po.se_kernel(p, ell, xm, fm, xm, fm, search=po.SEARCH_GRID)   # (the score's norm of the moving cloud: untransformed)
    sm = float(np.sum(Amm[2].astype(np.float64)))
    total = 0
    for label, R, T in hc.poses(xf):
        tag = "%s %s ell %g %s" % (name, mode_name, ell, label)
        y = po.transform(R, T, xm)
        A = po.se_kernel(p, ell, xf, ff, y, fm, search=po.SEARCH_GRID)
        rows = np.repeat(np.arange(n), np.diff(A[0]))
        cols, val = A[1], A[2]
        nnz = len(cols)
        total += nnz
        if name in hc.FAR:
            assert nnz > 0, tag
        # ---- flow and step
        c.transform_pcd(R, T)
        out = c.flow(ell)
        om, v, sa, sad2 = po.flow(p, ell, xf, y, A)
        assert int(out[8]) == nnz, (tag, int(out[8]), nnz)
        assert _close(out[0:3], om) and _close(out[3:6], v), (tag, out[0:6], om, v)
        assert _close([out[6]], [sa]) and _close([out[7]], [sad2]), tag
        omega, vv = om.astype(np.float32), v.astype(np.float32)
        assert np.array_equal(out[0:3].astype(np.float32), omega) and np.array_equal(out[3:6].astype(np.float32), vv), tag
        bcde = c.step_coeffs(omega, vv, ell)
        want = po.step_coeffs(ell, omega, vv, xf, y, A)
        assert _close(bcde, want, 1e-10), (tag, bcde, want)
        assert capi.pick_step(bcde) == po.pick_step(want), tag
        if acvo:
            Ayy = po.se_kernel(p, ell, y, fm, y, fm, search=po.SEARCH_GRID)
            assert (int(out[10]), int(out[12])) == (int(Axx[0][-1]), int(Ayy[0][-1])), tag
            assert _close([out[9]], [_self_sum(xf, Axx, 0, ell)], 1e-9), tag
            assert _close([out[11]], [_self_sum(y, Ayy, n, ell)], 1e-9) or (m <= n and out[11] == 0.0), tag
        # ---- per-row and per-column membership
        mt = c.pose_matches(R, T, ell)
        wantm = mref.from_members(rows, cols, val, n, m)
        wantm["members"] = (rows, cols, val)
        _check_matches(mt, wantm, tag)
        # ---- the counts against all-pairs distances in float64 (no search, no float32 d2)
        d2 = _all_pairs_d2(xf, y)
        inside, reach = d2 < tau * (1.0 - 1e-6), d2 < tau * (1.0 + 1e-6)
        band = int(reach.sum() - inside.sum())
        print("%s: nnz %d, pairs within 1e-6 of tau %d" % (tag, nnz, band))
        assert band <= 1e-3 * nnz, (tag, band, nnz)
        D = po.se_kernel(p, ell, xf, ff, y, fm, search=po.SEARCH_DENSE)   # (which pairs carry a weight: every pair looked at)
        weighted = np.zeros((n, m), bool)
        weighted[np.repeat(np.arange(n), np.diff(D[0])), D[1]] = True
        sure = inside & weighted
        assert np.all(mt.fixed.count >= sure.sum(1)) and np.all(mt.moving.count >= sure.sum(0)), tag
        assert np.all(mt.fixed.count <= reach.sum(1)) and np.all(mt.moving.count <= reach.sum(0)), tag
        assert not (weighted & ~reach).any(), tag
        # ---- score (and the matches' summary is the score's)
        s = c.pose_score(R, T, ell)
        a64 = val.astype(np.float64)
        inner = float(np.sum(a64))
        wants = dict(inner=inner, self_fixed=sf, self_moving=sm, nnz=nnz, nnz_fixed=len(Axx[1]), nnz_moving=len(Amm[1]),
                     cos_angle=inner / np.sqrt(sf * sm) if sf > 0 and sm > 0 else 0.0,
                     mean_d2=float(np.sum(a64 * ref.sq_dist(xf, y, rows, cols))) / inner if nnz else 0.0,
                     fixed_matched=len(np.unique(rows)), moving_matched=len(np.unique(cols)))
        _check_score(s, wants, tag)
        assert (mt.inner, mt.nnz, mt.fixed_matched, mt.moving_matched, mt.n_fixed, mt.n_moving, mt.ell) == \
            (s.inner, s.nnz, s.fixed_matched, s.moving_matched, s.n_fixed, s.n_moving, s.ell), tag
        assert s.n_fixed == n and s.n_moving == m and s.ell == np.float32(ell), tag
        # ---- Hessian
        if ell == HESS_ELL:
            h = c.pose_hessian(R, T, ell)
            wh = href.restate(xf, y, rows, cols, val, ell)
            assert h.nnz == nnz and abs(h.f - wh["f"]) <= 1e-11 * wh["f"], tag
            assert np.all(np.abs(h.g - wh["g"]) <= HESS_RTOL * wh["sg"]), (tag, h.g, wh["g"], wh["sg"])
            assert np.all(np.abs(h.H - wh["H"]) <= HESS_RTOL * wh["sH"]), (tag, np.abs(h.H - wh["H"]) / np.maximum(wh["sH"], 1e-300))
            assert np.array_equal(h.H, h.H.T), tag
            assert h.f == s.inner, tag
            if nnz == 0:
                assert h.f == 0.0 and not h.g.any() and not h.H.any(), tag
    c.close()
    if not name.startswith("tiny") and ell == hc.ELLS[0]:
        assert total > 0, name   # the case exercises something


@pytest.mark.parametrize("mode_name", MODES)
@pytest.mark.parametrize("name", hc.NAMES)
def test_pose_scan(pkg, po, name, mode_name):
    """cvo_hip_pose_scan over pose_scan_ref.accuracy_poses re-centred about the fixed cloud's box centre, against the
    restatement and against cvo_hip_pose_score at each pose (tests/test_gpu_pose_scan.py's tolerances: inner within the
    float64 sums' own bound 2 gamma(nnz), mean_d2 to 1e-6, cosines to 1e-10)."""
    acvo, mode, omode = _modes(pkg, po, mode_name)
    ell = 0.1
    xf, ff, xm, fm = hc.clouds(pkg.data, name, acvo)
    Rs, Ts = hc.scan_poses(xf, sref.accuracy_poses)
    c = _ctx(pkg, pkg.capi.default_params(mode), xf, ff, xm, fm)
    got = c.pose_scan(Rs, Ts, ell)
    scores = [c.pose_score(Rs[k], Ts[k], ell) for k in range(len(Rs))]
    c.close()
    want = sref.scan(po, omode, ell, xf, ff, xm, fm, Rs, Ts)
    print(name, mode_name, "nnz", got.nnz.tolist(), "best", got.best, want["best"])
    assert got.count == 25 and got.n_fixed == len(xf) and got.n_moving == len(xm) and got.ell == np.float32(ell)
    assert np.array_equal(got.nnz, want["nnz"])
    assert got.nnz_fixed == want["nnz_fixed"] and got.nnz_moving == want["nnz_moving"]
    assert want["nnz"][22] == 0 == want["nnz"][23]   # the two poses far away
    for k in range(25):
        g = sref.gamma(int(want["nnz"][k]))
        assert abs(got.inner[k] - want["inner"][k]) <= 2 * g * want["inner"][k], k
        assert abs(got.mean_d2[k] - want["mean_d2"][k]) <= 1e-6 * want["mean_d2"][k], k
        assert abs(got.cos_angle[k] - want["cos_angle"][k]) <= 1e-10, k
        if want["nnz"][k] == 0:
            assert got.inner[k] == 0.0 and got.mean_d2[k] == 0.0 and got.cos_angle[k] == 0.0, k
    assert got.best == want["best"]
    for k, s in enumerate(scores):
        g = sref.gamma(s.nnz)
        assert got.nnz[k] == s.nnz, k
        assert (got.self_fixed, got.self_moving, got.nnz_fixed, got.nnz_moving) == (s.self_fixed, s.self_moving, s.nnz_fixed, s.nnz_moving)
        assert abs(got.inner[k] - s.inner) <= 2 * g * s.inner, k
        assert abs(got.mean_d2[k] - s.mean_d2) <= (4 * g + 4 * sref.U) * s.mean_d2, k


def test_pose_score_many_over_every_case(pkg):
    """cvo_hip_pose_score_many over all the cases at once, cvo and acvo mixed: each struct is the lone call's, byte for byte."""
    capi = pkg.capi
    items = []
    for k, name in enumerate(hc.NAMES):
        for acvo in (False, True):
            cl = hc.clouds(pkg.data, name, acvo)
            label, R, T = hc.poses(cl[0])[(k + acvo) % 8]
            items.append((capi.default_params(capi.MODE_ACVO if acvo else capi.MODE_CVO), cl, R, T, hc.ELLS[k % 3]))
    ctxs = [_ctx(pkg, p, *cl) for p, cl, _, _, _ in items]
    try:
        lone = [bytes(c.pose_score_raw(R, T, ell)) for c, (_, _, R, T, ell) in zip(ctxs, items)]
        many = capi.pose_score_many_raw(ctxs, [it[2] for it in items], [it[3] for it in items], [it[4] for it in items])
        assert [bytes(s) for s in many] == lone
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------
# 4: the extremal stream of the bounding-sphere cull
# ---------------------------------------------------------------------------
CULL_TRIALS = 500   # per (offset, largest angle)


@pytest.mark.parametrize("cls", range(len(hc.CULL_CLASSES)))
def test_cull_loses_no_member_on_the_extremal_stream(pkg, po, cls):
    """Two collinear runs of 64 points whose nearest end points lie a hair inside or outside sqrt(tau) at the pose, far from
    the origin, under a small rotation about a random axis (hostile_cases.cull_trial): the pair of runs is one test of
    spheres_near (csrc/cvo_device.h), and a cull that drops it although the exact test has a member shows as a member count
    below the oracle's.  One context per offset class, the clouds re-set per trial, 3 x 500 trials; the same stream runs
    through the library's host-and-device code 21 000 times per class in tests/test_hostile_cpu.py, which is where the
    slack that ignored the coordinates lost 0.2 - 0.6 % of the trials from 600 m on."""
    capi = pkg.capi
    offset, gl, gh = hc.CULL_CLASSES[cls]
    p = po.default_params(po.MODE_CVO)
    ell = 0.1
    tau = po.thresholds(p, ell)[0]
    feat = np.ascontiguousarray(np.tile(np.array([120.0, 90.0, 150.0, 8.0, -5.0], np.float32), (64, 1)))
    c = capi.Context(mode=capi.MODE_CVO, device=0, stream=_stream())
    rng = np.random.Generator(np.random.PCG64(977 + cls))
    lost, with_member, trials = [], 0, 0
    for theta_max in hc.CULL_THETA_MAX:
        for _ in range(CULL_TRIALS):
            xf, xm, R, T = hc.cull_trial(rng, offset, gl, gh, theta_max, tau)
            c.set_fixed(xf, feat)
            c.set_moving(xm, feat)
            c.transform_pcd(R, T)
            got = int(c.flow(ell)[8])
            want = int(po.se_kernel(p, ell, xf, feat, po.transform(R, T, xm), feat, search=po.SEARCH_GRID)[0][-1])
            trials += 1
            with_member += want > 0
            if got != want:
                lost.append((theta_max, trials, got, want))
    c.close()
    print("offset %s: %d trials, %d with a member, %d differ" % (offset, trials, with_member, len(lost)))
    assert 2 * with_member >= trials, (with_member, trials)
    assert not lost, (len(lost), lost[:10])


# ---------------------------------------------------------------------------
# 5a: registrations
# ---------------------------------------------------------------------------
_ORACLE_ALIGN = {}


def _oracle_align(po, pkg, name, acvo):
    key = (name, acvo)
    if key not in _ORACLE_ALIGN:
        p = po.default_params(po.MODE_ACVO if acvo else po.MODE_CVO)
        st = po.init_state(p)
        n_or, tr = po.align(p, st, *hc.clouds(pkg.data, name, acvo), search=po.SEARCH_GRID, trace_cap=2000)
        _ORACLE_ALIGN[key] = (n_or, tr, bytes(st))
    return _ORACLE_ALIGN[key]


def _lone_context(pkg, mode, clouds, list_init=0):
    import torch
    s = torch.cuda.Stream()
    c = pkg.capi.Context(mode=mode, device=0, stream=s.cuda_stream, graph_capture=True)
    if list_init:
        c.set_option("list_init", list_init)   # every list starts at this capacity (its minimum at least)
    c.set_fixed(clouds[0], clouds[1])
    c.set_moving(clouds[2], clouds[3])
    return c, s


@pytest.mark.parametrize("mode_name", MODES)
@pytest.mark.parametrize("name", hc.NAMES)
def test_align_matches_oracle(pkg, po, name, mode_name):
    """A registration of every case on its own: the trace of every iteration (nnz, ell, omega, v, step) and the whole state
    equal the oracle's, with the candidate record narrowed or rebuilt and with resident runs allowed or denied.  (far*: 1 - 7
    iterations, see the module docstring.)"""
    acvo, mode, _ = _modes(pkg, po, mode_name)
    capi = pkg.capi
    n_or, tr_or, st_or = _oracle_align(po, pkg, name, acvo)
    c, s = _lone_context(pkg, mode, hc.clouds(pkg.data, name, acvo))
    for narrow in (1, 0):
        for runs in (1, 0):
            c.set_option("record_narrow", narrow)
            c.set_option("resident_runs", runs)
            st = capi.init_state(c.params)
            n_it, tr = c.align(st, trace_cap=2000)
            tag = (name, mode_name, narrow, runs)
            print(tag, "iterations", n_it, "list_stats", c.list_stats(), "run_stats", c.run_stats())
            assert n_it == n_or, (tag, n_it, n_or)
            for k, (a, b) in enumerate(zip(tr, tr_or)):
                assert a["nnz"] == b["nnz"] and a["ell"] == b["ell"], (tag, k, a["nnz"], b["nnz"])
                assert a["omega"] == b["omega"] and a["v"] == b["v"] and a["step"] == b["step"], (tag, k)
            assert bytes(st) == st_or, tag
    c.close()


@pytest.mark.parametrize("mode_name", MODES)
def test_blob_from_the_smallest_lists(pkg, po, mode_name):
    """`blob` with every list started at its minimum capacity (test switch "list_init"): the loop parks on an overflowed
    list, the host grows it and resumes (cvo_job.cpp), and the registration is still the oracle's.  At the default capacities
    `blob` overflows nothing -- the tile lists start at four entries per 16 x 16 tile, the kept list at 2^20 members against
    the 706 800 (cvo) / 190 357 (acvo) of this case -- so the growth is FORCED here, and the context's read-only counter
    "list_grows" says that it happened."""
    acvo, mode, _ = _modes(pkg, po, mode_name)
    capi = pkg.capi
    n_or, tr_or, st_or = _oracle_align(po, pkg, "blob", acvo)
    c = capi.Context(mode=mode, device=0, stream=_stream())
    c.set_option("list_init", 1)
    xf, ff, xm, fm = hc.clouds(pkg.data, "blob", acvo)
    c.set_fixed(xf, ff)
    c.set_moving(xm, fm)
    st = capi.init_state(c.params)
    n_it, tr = c.align(st, trace_cap=2000)
    grows = c.get_option("list_grows")
    c.close()
    print("blob", mode_name, "list_grows", grows)
    assert grows >= 1
    assert n_it == n_or and [t["nnz"] for t in tr] == [t["nnz"] for t in tr_or]
    assert bytes(st) == st_or


def test_align_many_mixed_bag_matches_oracle(pkg, po):
    """Every case, cvo and acvo, in ONE cvo_hip_align_many call -- tiny clouds beside a blob whose lists overflow, a jump whose
    lists die young beside clouds 1.5 km away -- with the record narrowed or rebuilt and resident runs allowed or denied:
    iteration counts and whole states equal the oracle's.  The counters show that the cases do what they are for.  `blob`
    starts from lists of the minimum capacity (test switch "list_init" on its two contexts; at the default capacities it
    overflows nothing, see test_blob_from_the_smallest_lists): its registrations park inside the engines, their lists grow
    (cvo_engine.cpp) and "list_grows" counts it.  `jump`: more than one all-pairs build and fewer builds than iterations
    (cvo_hip_get_list_stats) -- lists were re-used and lists were rebuilt; the counters do not say in which order, but the
    first iteration always builds, so a second build with re-use anywhere means the list of some build died."""
    capi = pkg.capi
    keys = [(name, acvo) for name in hc.NAMES for acvo in (False, True)]
    made = [_lone_context(pkg, capi.MODE_ACVO if acvo else capi.MODE_CVO, hc.clouds(pkg.data, name, acvo), list_init=name == "blob")
            for name, acvo in keys]
    ctxs = [m[0] for m in made]
    want = [_oracle_align(po, pkg, name, acvo) for name, acvo in keys]
    try:
        for narrow, runs in ((1, 1), (0, 1), (1, 0), (0, 0)):
            for c in ctxs:
                c.set_option("record_narrow", narrow)
                c.set_option("resident_runs", runs)
            states = [capi.init_state(c.params) for c in ctxs]
            its = capi.align_many(ctxs, states)
            stats = {k: c.list_stats() for k, c in zip(keys, ctxs)}
            print("narrow %d runs %d: blob %s %s, jump %s %s" % (narrow, runs, stats[("blob", False)], stats[("blob", True)],
                                                                  stats[("jump", False)], stats[("jump", True)]))
            for k, it, st, w in zip(keys, its, states, want):
                assert it == w[0], (k, narrow, runs, it, w[0])
                assert bytes(st) == w[2], (k, narrow, runs)
            for acvo in (False, True):
                builds = stats[("jump", acvo)][0]
                assert 2 <= builds < want[keys.index(("jump", acvo))][0], (acvo, stats[("jump", acvo)])   # a rebuild after a re-use
                grows = ctxs[keys.index(("blob", acvo))].get_option("list_grows")
                print("blob acvo %d: list_grows %d" % (acvo, grows))
                assert grows >= 1, (acvo, grows)
    finally:
        for c in ctxs:
            c.close()
