"""CPU: the oracle's O(N.M) arithmetic (oracle/cvo_oracle.c: se_kernel, compute_flow, acvo's dl, function_inner_product,
compute_step_size) against the float64 restatement of the reference's formulae in tests/cvo_iteration_ref.py.

Every tolerance is derived in tests/iteration_ref_cases.py's docstring (K roundings of float32, u = 2^-24, times the sum
of the absolute products) and none is fitted to an observed error.  Sums are compared over the oracle's OWN member set
with the float64 weights, so that a borderline pair cannot hide in a tolerance; the member set itself is held apart:
every pair surely inside the three cuts is a member, no pair surely outside is one.

Cases: data.synthetic_pair(n, m, seed=11) at the five sizes of iteration_ref_cases.SIZES, modes cvo, acvo and the MATLAB
weight (dense search), ell in {0.15, 0.1, 0.06, 0.03}, three poses (identity, a small motion, about one ell away); and two
more acvo parameter sets (iteration_ref_cases.ACVO_VARIANTS) under which the radius and the colour cut -- both implied by
a > sp_thres at the shipped constants -- decide pairs of their own.  Every test prints its worst error as a fraction of the
tolerance (pytest -s); DESIGN.md section 2 records them.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvo_iteration_ref as ref  # noqa: E402
import iteration_ref_cases as ic  # noqa: E402
import pose_hessian_ref  # noqa: E402
import pose_score_ref  # noqa: E402

U = ic.U
VISIBLE = 10.0   # a term is visible in a case when it exceeds this many tolerances of its sum


def _rows(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def _member_record(margin, rows, cols):
    """How the oracle's member set (rows, cols) sits in the reference's three classes."""
    sure_in, border, sure_out = ref.classify(margin)
    mask = np.zeros(margin.shape, bool)
    mask[rows, cols] = True
    return dict(nnz=len(rows), sure_in=int(sure_in.sum()), border=int(border.sum()),
                missing=int((sure_in & ~mask).sum()), extra=int((sure_out & mask).sum()))


def _case(pkg, po, mode, n, m, ell, pose, over=None):
    """One case: everything the oracle computes for it next to the reference, as error / tolerance ratios."""
    name, R, T = pose
    xf, ff, xm, fm = ic.clouds(pkg, mode, n, m)
    p = po.default_params(ic.mode_id(po, mode))
    for key, value in (over or {}).items():
        setattr(p, key, value)
    search = po.SEARCH_DENSE if mode == "matlab" else po.SEARCH_GRID
    y = po.transform(R, T, xm)
    rp, cols, val = po.se_kernel(p, ell, xf, ff, y, fm, search=search)
    rows = _rows(rp)
    a, d2, d2c, margin = ref.weights(p, ell, xf, ff, y, fy=fm, c_sp=ic.c_sp_of(p))
    rec = dict(mode=mode, n=n, m=m, ell=ell, pose=name, over=over, members=_member_record(margin, rows, cols))
    am = a[rows, cols]
    bound = ic.weight_bound(p, ell, am, d2[rows, cols], d2c[rows, cols])
    rec["weight"] = float(np.max(np.abs(val - am) / bound)) if len(rows) else 0.0
    rec["weight_rel"] = float(np.max(np.abs(val - am) / am)) if len(rows) else 0.0
    rec["weight_bound_rel"] = float(np.max(bound / am)) if len(rows) else 0.0
    # which cut decides: pairs that one cut alone removes (the other two passed) -- the cut is exercised
    if p.color_scale == 0:
        tau, tau_c = ref.cuts(p, ell, ic.c_sp_of(p))
        sp = float(np.float32(p.sp_thres))
        rec["cut_alone"] = dict(d2=int(((d2 >= tau) & (d2c < tau_c) & (a > sp)).sum()),
                                d2c=int(((d2 < tau) & (d2c >= tau_c) & (a > sp)).sum()),
                                a=int(((d2 < tau) & (d2c < tau_c) & (a <= sp)).sum()))
    # compute_flow
    om, v, sa, sad2 = po.flow(p, ell, xf, y, (rp, cols, val))
    fl = ref.flow(p, ell, xf, y, rows, cols, am)
    tol = ic.flow_tol(p, fl)
    got = dict(omega_d=om, v_d=v, sum_a=sa, sum_a_d2=sad2)
    with np.errstate(divide="ignore", invalid="ignore"):
        rec["flow"] = {k: np.max(np.nan_to_num(np.abs(got[k] - fl[k]) / tol[k])) for k in got}
        rec["flow_visible"] = {k: np.nan_to_num(np.abs(fl[k]) / tol[k]) for k in got}
    # compute_step_size: the flow's own twist and three synthetic ones
    omega, vv = om.astype(np.float32), v.astype(np.float32)
    rec["step"] = []
    for s, w_, v_ in [(0.0, omega, vv)] + ic.twists(seed=n * 1000 + m):
        bcde = po.step_coeffs(ell, w_, v_, xf, y, (rp, cols, val))
        st = ref.step_terms(ell, w_, v_, xf, y, rows, cols, am)
        stol = ic.step_tol(p, st)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = dict(s=s, err=np.nan_to_num(np.abs(bcde - st["bcde"]) / stol),
                     visible={t: float(np.nan_to_num(abs(st["terms"][t]) / stol[ref.COEFF_OF[t.split(".")[0]]]))
                              for t in ref.STEP_TERMS + ref.SUB_TERMS})
            if s == 0.0:   # B = (c omega.omega_d + d v.v_d) / l^2 on the oracle's outputs
                l2 = float(np.float32(ell)) ** 2
                ident = (float(p.c) * np.dot(omega.astype(np.float64), om) + float(p.d) * np.dot(vv.astype(np.float64), v)) / l2
                r["identity"] = float(np.nan_to_num(abs(bcde[0] - ident) / stol[0]))
                r["identity_rel"] = float(np.nan_to_num(abs(bcde[0] - ident) / abs(ident)))
        rec["step"].append(r)
    if mode == "acvo":
        # function_inner_product on the untransformed clouds (its own thresholds), and dl from a one-iteration trace
        fip = po.function_inner_product(p, ell, xf, ff, xm, fm, search=search)
        want, s_keep, n_keep, fmargin = ref.function_inner_product(p, ell, xf, ff, xm, fm)
        nb = int(ref.classify(fmargin)[1].sum())
        rec["fip"] = dict(got=fip, want=want, n=n_keep, border=nb, tol=(ic.kw(p) + 1) * U * abs(want) if n_keep else 0.0)
        # the same with the colour cut taken from c_sp_thres, as acvo's se_kernel forms it: how far the wrong choice is
        a2, _, _, m2 = ref.weights(p, ell, xf, ff, xm, fm, c_sp=p.c_sp_thres, two_divisions=True)
        rec["fip"]["other"] = float(a2[m2 < 0].sum() / max(int((m2 < 0).sum()), 1))
        q = po.default_params(po.MODE_ACVO)
        for key, value in (over or {}).items():
            setattr(q, key, value)
        q.ell_init, q.max_iter = ell, 1
        st_ = po.init_state(q)
        st_.R[:] = [float(t) for t in R.reshape(9)]
        st_.T[:] = [float(t) for t in T]
        _, tr = po.align(q, st_, xf, ff, xm, fm, search=search)
        A = (rows, cols, am)
        sets = {}
        for key, (pa, fa) in (("xx", (xf, ff)), ("yy", (y, fm))):
            rp2, c2, v2 = po.se_kernel(p, ell, pa, fa, pa, fa, search=search)
            r2 = _rows(rp2)
            a_s, d2_s, d2c_s, m_s = ref.weights(p, ell, pa, fa, pa, fa, c_sp=ic.c_sp_of(p))
            sets[key] = (r2, c2, a_s[r2, c2])
            rec["members_" + key] = _member_record(m_s, r2, c2)
        d = ref.dl(ell, xf, y, A, sets["xx"], sets["yy"])
        dtol = ic.dl_tol(p, d)
        t0 = tr[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            rec["dl"] = _dl_record(t0, d, dtol, fl, tol, (len(rows), len(sets["xx"][0]), len(sets["yy"][0])))
    return rec


def _dl_record(t0, d, dtol, fl, tol, counts):
    return dict(got=t0["dl"], want=d["dl"], tol=dtol, den=d["den"], counts=(t0["nnz"], t0["nnz_xx"], t0["nnz_yy"]) == counts,
                visible={k: float(np.nan_to_num(d[k] / abs(d["den"]) / dtol)) if d["den"] else 0.0
                         for k in ("s_yy", "s_xy", "s_xx", "s_yy_main")},
                trace_flow=max(np.max(np.nan_to_num(np.abs(np.array(t0["omega_d"]) - fl["omega_d"]) / tol["omega_d"])),
                               np.max(np.nan_to_num(np.abs(np.array(t0["v_d"]) - fl["v_d"]) / tol["v_d"]))))


@pytest.fixture(scope="module")
def records(pkg, po):
    out = []
    for mode in ic.MODES:
        for n, m in ic.SIZES:
            for ell in ic.ELLS:
                for pose in ic.poses(ell):
                    out.append(_case(pkg, po, mode, n, m, ell, pose))
    for over, ells in ic.ACVO_VARIANTS:
        for n, m in ((300, 260), (260, 300)):
            for ell in ells:
                for pose in ic.poses(ell):
                    out.append(_case(pkg, po, "acvo", n, m, ell, pose, over=over))
    return out


def _tag(r):
    return "%s %dx%d ell=%g %s %s" % (r["mode"], r["n"], r["m"], r["ell"], r["pose"], r["over"] or "")


def test_members_sit_between_surely_in_and_surely_out(records):
    """The oracle's CSR holds every pair surely inside the three cuts and none surely outside (|margin| > 1e-5); the
    borderline pairs are at most 1 per 1000 members -- a condition on the inputs: zero on every case here.  Per mode, at
    least three cases have more than 100 members and at least one is empty; every one of the three cuts removes, in some
    case, pairs that the other two would have kept."""
    for r in records:
        for key in ("members", "members_xx", "members_yy"):
            if key in r:
                mr = r[key]
                assert mr["missing"] == 0 and mr["extra"] == 0, (_tag(r), key, mr)
                assert mr["border"] * 1000 <= mr["nnz"], (_tag(r), key, mr)
                assert mr["sure_in"] <= mr["nnz"] <= mr["sure_in"] + mr["border"]
    for mode in ic.MODES:
        nn = [r["members"]["nnz"] for r in records if r["mode"] == mode]
        assert sum(k > 100 for k in nn) >= 3 and sum(k == 0 for k in nn) >= 1, (mode, sorted(nn))
    for cut in ("d2", "d2c", "a"):
        assert any(r["cut_alone"][cut] > 0 for r in records if "cut_alone" in r), cut
    print("borderline pairs over all cases:", sum(r["members"]["border"] for r in records))


def test_weights_within_the_derived_bound(records):
    """val against a at the oracle's members, per pair: |val - a| <= u (5 + 5 E1 + 7 E2) a for the C++ weight and
    u (7 + 5 E1) a for the MATLAB weight (iteration_ref_cases: five / seven roundings, and the float32 error of d2 and d2c
    -- 5 u and 7 u relative -- times the exponents' magnitudes E1 = d2 / 2 l^2, E2 = d2c / 2 c_l^2, which the cuts bound by
    ln(s2 cs2 / sp) together).  Relative, at the shipped constants: at most u (5 + 7 ln(s2 cs2 / sp)) = 3.9e-7 (cvo) and 3.8e-7
    (acvo), u (7 + 5 ln(s2 / sp)) = 1.1e-6 (MATLAB)."""
    worst = {}
    for r in records:
        assert r["weight"] <= 1.0, (_tag(r), r["weight"], r["weight_rel"])
        w = worst.setdefault(r["mode"], [0.0, 0.0, 0.0])
        worst[r["mode"]] = [max(w[0], r["weight"]), max(w[1], r["weight_rel"]), max(w[2], r["weight_bound_rel"])]
    print("weights: worst (error / bound, relative error, relative bound) per mode:", worst)


def test_flow_sums_within_k_roundings(records):
    """po.flow against the reference over the oracle's members with the float64 weights: omega_d (KW + 5), v_d (KW + 4),
    sum_a (KW), sum_a_d2 (KW + 10) roundings times u times the sum of absolute products (iteration_ref_cases).  Each of
    the four is visible -- more than ten tolerances large -- in some case, component by component."""
    worst = {}
    vis = {}
    for r in records:
        for k, e in r["flow"].items():
            assert e <= 1.0, (_tag(r), k, e)
            worst[k] = max(worst.get(k, 0.0), float(e))
            vis[k] = np.maximum(vis.get(k, 0.0), r["flow_visible"][k])
    for k, x in vis.items():
        assert np.all(x > VISIBLE), (k, x)
    print("flow: worst error / tolerance:", worst, " largest value / tolerance:", {k: np.round(x) for k, x in vis.items()})


def test_step_coefficients_within_k_roundings(records):
    """po.step_coeffs against the reference's B, C, D, E for the flow's own twist and omega, v ~ N(0, s), s in
    {0.02, 0.3, 1.0}: each coefficient within u sum_terms K_term S_term (iteration_ref_cases).  Each of the eleven products
    of cvo.cpp:275-279 (1 + 2 + 3 + 5) and each inner summand of gamma, delta and epsil (cvo.cpp:264-271) exceeds ten
    tolerances of its coefficient in some case: a dropped or mis-scaled term fails.  One summand cannot be made visible in
    any case: delta's xiz.xi2z is identically zero, because xi2z = omega_hat xiz and u.(omega cross u) = 0.  It is asserted
    to BE zero (below one tolerance of D everywhere) instead; the reference's line and the oracle carry it all the same."""
    worst = np.zeros(4)
    vis = {}
    for r in records:
        for s in r["step"]:
            assert np.all(s["err"] <= 1.0), (_tag(r), s["s"], s["err"])
            worst = np.maximum(worst, s["err"])
            for t, x in s["visible"].items():
                vis[t] = max(vis.get(t, 0.0), x)
    for t in ref.STEP_TERMS + ref.SUB_TERMS:
        if t == "D_delta.xiz_xi2z":   # identically zero: see the docstring
            assert vis[t] < 1.0
            continue
        assert vis[t] > VISIBLE, (t, vis[t])
    print("step: worst error / tolerance (B, C, D, E):", worst, " largest term / tolerance:", {t: round(x) for t, x in vis.items()})


def test_b_is_the_twist_against_the_flow(records):
    """B = (c omega.omega_d + d v.v_d) / l^2 with omega, v the float32-rounded twist (from xiz.(x - y) =
    -omega.(x cross y) - v.(y - x)), on the oracle's outputs, at B's tolerance.  (The right side carries the flow's own
    float32 rounding, relative to |x||y| where B's is relative to |y||x - y|; B's tolerance holds all the same, the worst case
    at 0.73 of it.  A swapped operand or a wrong 1/c, 1/d or 1/l^2 on either side is off by the whole of B.)"""
    worst = worst_rel = 0.0
    for r in records:
        s = r["step"][0]
        assert s["identity"] <= 1.0, (_tag(r), s["identity"], s["identity_rel"])
        worst, worst_rel = max(worst, s["identity"]), max(worst_rel, s["identity_rel"])
    print("B identity: worst error / tolerance %.3g, relative %.3g" % (worst, worst_rel))


def test_function_inner_product(records):
    """po.function_inner_product (acvo) against the reference: the mean of the kept weights, within (KW + 1) u of it (the
    weights' KW, the float result's rounding) where no pair is borderline.  With c_sp_thres = 0.98 the colour cut of
    acvo's se_kernel would keep a different set: function_inner_product must not follow it (adaptive_cvo.cpp:392)."""
    n_checked = n_told_apart = 0
    worst = 0.0
    for r in records:
        if "fip" not in r:
            continue
        f = r["fip"]
        assert f["border"] == 0, (_tag(r), f)
        if f["n"] == 0:
            assert np.isnan(f["got"]) and np.isnan(f["want"])
            continue
        assert abs(f["got"] - f["want"]) <= f["tol"], (_tag(r), f)
        n_checked += 1
        n_told_apart += abs(f["other"] - f["want"]) > VISIBLE * f["tol"]
        worst = max(worst, abs(f["got"] - f["want"]) / f["tol"])
    assert n_checked >= 20 and n_told_apart >= 12, (n_checked, n_told_apart)   # every case of the c_sp_thres variant
    print("function_inner_product: worst error / tolerance %.3g over %d cases, %d tell the two colour cuts apart"
          % (worst, n_checked, n_told_apart))


def test_dl_and_its_row_rule(records):
    """dl of record 0 of a one-iteration po.align against the reference on the oracle's three member sets: within
    (KW + 10) u (S_yy + 2 S_xy + S_xx) / |den|.  The record's counts are the sets' sizes and its omega_d, v_d the flow's.
    Each of the three contributions is visible in some case -- S_yy, the N <= i < M tail, only where M > N; what the
    main-loop rows of Ayy would add if they counted is visible too, so the quirk cannot be lost either way."""
    vis = {}
    n_checked = 0
    worst = 0.0
    for r in records:
        if "dl" not in r:
            continue
        d = r["dl"]
        assert d["counts"], _tag(r)
        assert d["trace_flow"] <= 1.0, (_tag(r), d["trace_flow"])
        if d["den"] == 0:
            assert not np.isfinite(d["got"]) and not np.isfinite(d["want"]), (_tag(r), d)
            continue
        assert abs(d["got"] - d["want"]) <= d["tol"], (_tag(r), d)
        worst = max(worst, abs(d["got"] - d["want"]) / d["tol"] if d["tol"] > 0 else 0.0)
        n_checked += 1
        for k, x in d["visible"].items():
            vis[k] = max(vis.get(k, 0.0), x)
        if r["m"] <= r["n"]:
            assert d["visible"]["s_yy"] == 0.0
    assert n_checked >= 20
    for k in ("s_yy", "s_xy", "s_xx", "s_yy_main"):
        assert vis[k] > VISIBLE, (k, vis[k])
    print("dl: worst error / tolerance %.3g;" % worst, "largest contribution / tolerance:", {k: round(x) for k, x in vis.items()})


def test_transform_is_the_inverse_pose(po, pkg):
    """po.transform (update_tf + transform_pcd, cvo.cpp:83-87,310-315) against R^T (y - T) in float64: -R^T T is three
    products and two additions (K = 3), a point three products, two additions and the translation (K = 4):
    4 u (|R^T| |y| + |R^T| |T|) per component."""
    xm = pkg.data.synthetic_pair(64, 300, seed=11)[2]
    for _, R, T in ic.poses(0.15):
        y = po.transform(R, T, xm).astype(np.float64)
        R64, T64, Y0 = R.astype(np.float64), T.astype(np.float64), xm.astype(np.float64)
        want = (Y0 - T64) @ R64
        tol = 4 * U * (np.abs(Y0) @ np.abs(R64) + np.abs(T64) @ np.abs(R64))
        assert np.all(np.abs(y - want) <= tol)


def test_pose_query_references_rest_on_checked_weights(pkg, po):
    """pose_score_ref.score's inner and nnz, and the f and g that tests/test_gpu_pose_hessian.py obtains from
    pose_hessian_ref.restate on the oracle's members, against the new reference: the member count equal (no borderline
    pair in this case), inner and f within KW u sum a of sum_a, g within KW u of the twist sums scaled back by c, d and
    l^2 (both modules add the oracle's float32 weights in float64: the weights' error is all there is)."""
    n, m, ell = 300, 260, 0.1
    xf, ff, xm, fm = ic.clouds(pkg, "cvo", n, m)
    _, R, T = ic.poses(ell)[1]
    p = po.default_params(po.MODE_CVO)
    y = po.transform(R, T, xm)
    a, _, _, margin = ref.weights(p, ell, xf, ff, y, fm, c_sp=ic.c_sp_of(p))
    assert int(ref.classify(margin)[1].sum()) == 0
    rows, cols = ic.dense_members(p, margin)
    assert len(rows) > 100
    fl = ref.flow(p, ell, xf, y, rows, cols, a[rows, cols])
    k = ic.kw(p)
    sc = pose_score_ref.score(po, po.MODE_CVO, ell, xf, ff, xm, fm, R, T)
    assert sc["nnz"] == len(rows)
    assert abs(sc["inner"] - fl["sum_a"]) <= k * U * fl["s_a"]
    rp, col, val = po.se_kernel(p, ell, xf, ff, y, fm, search=po.SEARCH_GRID)
    h = pose_hessian_ref.restate(xf, y, _rows(rp), col, val, ell)
    l2 = float(np.float32(ell)) ** 2
    assert h["nnz"] == len(rows)
    assert abs(h["f"] - fl["sum_a"]) <= k * U * fl["s_a"]
    # (restate takes ell as the Python float it is given; float32(0.1) differs from it by 1.5e-8 relative: one more u)
    assert np.all(np.abs(h["g"][:3] - p.c * fl["omega_d"] / l2) <= (k + 1) * U * p.c * fl["s_omega"] / l2)
    assert np.all(np.abs(h["g"][3:] - p.d * fl["v_d"] / l2) <= (k + 1) * U * p.d * fl["s_v"] / l2)
