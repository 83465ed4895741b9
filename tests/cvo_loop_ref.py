"""Float64 restatement of the O(1) half of a CVO / Adaptive-CVO iteration -- "the head": what turns the reduced sums of
an iteration into the next state -- and a replay of a registration's own trace with it.

Reference lines followed (paths under cpp/rkhs_registration/):
    src/cvo.cpp:291-307            the step from the cubic        src/cvo.cpp:380, adaptive_cvo.cpp:509   break A
    src/LieGroup.cpp:159-186       Exp_SEK3                       src/cvo.cpp:71-81                       dist_se3
    src/cvo.cpp:398-399            the update of R, T             src/cvo.cpp:402, adaptive_cvo.cpp:531   break B
    src/cvo.cpp:408-410            cvo's length-scale schedule    src/adaptive_cvo.cpp:538-545            acvo's rule
    src/cvo.cpp:413-415, 83-87     prev / accum / transform       src/adaptive_cvo.cpp:476-477            acvo's reset of ell
TOLERANCE, the small-angle threshold of Exp_SEK3, is declared in include/LieGroup.h:21 (extern const float) and defined
in src/LieGroup.cpp:18 as 1e-6.

A plain module shared by tests/test_loop_ref_cpu.py (the oracle against this) and tests/test_gpu_loop_ref.py (the
library's heads against this).  It knows nothing of the oracle or the library: numpy float64 and scipy.linalg only.  A
trace record carries the head's inputs (omega, v, bcde, dl, k) as the float32 / float64 values the head itself read, so
every record is judged from its own inputs; only the length scale and the pose are walked from the state the registration
began with.  The functions are gathered in RULES: the mutants of tests/loop_ref_cases.py replace one at a time.
"""
import types

import numpy as np
import scipy.linalg

from iteration_ref_cases import cubic_roots, roots_step

U = 2.0 ** -24
TOLERANCE = np.float32(1e-6)      # src/LieGroup.cpp:18
STEP_MAX = np.float32(0.8)        # src/cvo.cpp:307 (compared and assigned as double 0.8, stored in a float)
A_BAND_CVO = 3.0 * U              # a float32 norm: three squares, two additions (3 u of the sum), the root (halved, + 1): < 3 u
A_BAND_ACVO = 1e-12               # double norms of the float vectors
THETA_BAND = 3.0 * U              # the float32 norm Exp_SEK3 compares with TOLERANCE: the same count

CENSUS_KEYS = ("step_clamped", "step_unclamped", "step_min", "step_min_late", "small_angle", "break_a", "break_b", "max_iter", "shrink", "floor",
               "schedule_3", "schedule_10", "schedule_20")
CONDITION_KEYS = ("borderline_a", "borderline_theta", "step_skipped")


def _f(v):
    return np.asarray(v, np.float32).astype(np.float64)


def mode_of(p):
    return "acvo" if p.mode == 1 else "cvo"


def step(bcde, min_step):
    """cvo.cpp:291-307: the smallest positive real root of 4E t^3 + 3D t^2 + 2C t + B (coefficients cast to float),
    min_step where there is none, and 0.8 where either exceeds 0.8.  A degenerate cubic -- E == 0 as a float, or a
    coefficient that is not finite -- has a companion matrix that is not finite (poly_solver divides by coef(0)): no root
    passes the test of :300 and the step is min_step, clamped.  None only for a nearly double root (roots_step)."""
    if cubic_roots(bcde) is None:
        want = np.float32(min_step)
        return float(STEP_MAX if want > 0.8 else want)
    return roots_step(bcde, np.float32(min_step))


def stops_on_twist(mode, omega, v, eps):
    """Break A: |omega| < eps && |v| < eps.  cvo (cvo.cpp:380) takes float32 norms, acvo (adaptive_cvo.cpp:509) double norms
    of the float vectors.  Returns (verdict, borderline): borderline when a norm that the verdict depends on lies within
    the band of eps -- the rounding of a float32 norm (A_BAND_CVO), 1e-12 relative for acvo."""
    eps = float(np.float32(eps))
    band = (A_BAND_ACVO if mode == "acvo" else A_BAND_CVO) * eps
    below, near = [], []
    for vec in (omega, v):
        n = float(np.sqrt(np.sum(_f(vec) ** 2)))
        below.append(n < eps)
        near.append(abs(n - eps) <= band)
    verdict = below[0] and below[1]
    borderline = (near[0] and (below[1] or near[1])) or (near[1] and (below[0] or near[0]))
    return verdict, borderline


def theta32(omega):
    """(|omega| as Exp_SEK3 sees it, borderline): the float32 norm against TOLERANCE."""
    n = float(np.sqrt(np.sum(_f(omega) ** 2)))
    return n, abs(n - float(TOLERANCE)) <= THETA_BAND * float(TOLERANCE)


def small_angle(omega):
    return theta32(omega)[0] < float(TOLERANCE)


def exp_sek3(omega, v, dt):
    """LieGroup.cpp:159-186 with K = 1: (dR, dT) of expm(dt [omega^ v; 0 0]); and its small-angle branch (:168-170), float32
    |omega| < TOLERANCE: R = I and Jl = I, so dT = v -- NOT scaled by dt."""
    w, vv, dt = _f(omega), _f(v), float(np.float32(dt))
    if small_angle(omega):
        return np.eye(3), vv.copy()
    xi = np.zeros((4, 4))
    xi[:3, :3] = skew(w)
    xi[:3, 3] = vv
    X = scipy.linalg.expm(dt * xi)
    return X[:3, :3], X[:3, 3]


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def dist(dR, dT):
    """cvo.cpp:71-81: the Frobenius norm of logm([dR dT; 0 1])."""
    M = np.eye(4)
    M[:3, :3] = dR
    M[:3, 3] = dT
    return float(np.linalg.norm(np.real(scipy.linalg.logm(M))))


def dist_arguments(dR, dT, R, T):
    """dist_se3 is called on the increment (cvo.cpp:402), not on the updated pose."""
    return dR, dT


def update(R, T, dR, dT):
    """cvo.cpp:398-399: T = R dT + T with the OLD R, then R = R dR."""
    return R @ dR, R @ dT + T


def next_ell(mode, k, ell, ell_max, dl, p):
    """The length scale after iteration k, float32-exact with the C promotions spelt out.
    cvo (cvo.cpp:408-410): ell = (k > 2) ? 0.10 : ell and so on -- a double constant stored in a float.
    acvo (adaptive_cvo.cpp:538-545): ell = (float)((double)ell + dl_step * dl); if (ell >= ell_max) both become
    (float)((double)ell_max * 0.7), from the OLD ell_max; then the floor ell_min."""
    ell, ell_max = np.float32(ell), np.float32(ell_max)
    if mode == "acvo":
        with np.errstate(all="ignore"):
            ell = np.float32(float(ell) + float(p.dl_step) * float(dl))
        if ell >= ell_max:
            shrunk = np.float32(float(ell_max) * 0.7)
            ell, ell_max = shrunk, shrunk
        if ell < np.float32(p.ell_min):
            ell = np.float32(p.ell_min)
        return ell, ell_max
    if k > 2:
        ell = np.float32(0.10)
    if k > 9:
        ell = np.float32(0.06)
    if k > 19:
        ell = np.float32(0.03)
    return ell, ell_max


def ell_after(rules, mode, k, ell, ell_max, dl, p, exit_code):
    """Both breaks leave the loop before the length-scale lines: they apply only when neither fired."""
    if exit_code != 0:
        return np.float32(ell), np.float32(ell_max)
    return rules.next_ell(mode, k, ell, ell_max, dl, p)


def final_iter(iter0, break_k, max_iter):
    """`iter = k` is written at a break only (cvo.cpp:381,403): a loop that max_iter ends leaves iter as it was."""
    return iter0 if break_k is None else break_k


def tf_of(R, T):
    """update_tf (cvo.cpp:83-87): [R' | -R' T; 0 0 0 1]."""
    M = np.eye(4)
    M[:3, :3] = R.T
    M[:3, 3] = -R.T @ T
    return M


def finish(state0, used_transform, R, T):
    """cvo.cpp:413-415: prev_transform = the transform in use -- that of the top of the last executed iteration, the one
    the state came in with when none was executed; accum_transform = accum_transform * that; then update_tf() on the final
    R, T.  Returns (transform, prev_transform, accum_transform) in float64."""
    used = np.asarray(used_transform, np.float64)
    return tf_of(R, T), used, np.asarray(state0["accum_transform"], np.float64) @ used


RULES = types.SimpleNamespace(step=step, stops_on_twist=stops_on_twist, exp_sek3=exp_sek3, dist=dist, dist_arguments=dist_arguments, update=update,
                              next_ell=next_ell, ell_after=ell_after, final_iter=final_iter, finish=finish)


def with_rule(**changed):
    """RULES with some functions replaced (the mutants)."""
    d = dict(vars(RULES))
    d.update(changed)
    return types.SimpleNamespace(**d)


def replay(p, state0, trace, rules=None):
    """Walks the records of one align() from the state it began with.  state0: dict of float32 arrays R (3, 3), T (3,),
    transform / prev_transform / accum_transform (4, 4) and ell, ell_max, iter.  Every record is judged from its own
    omega, v, bcde, dl and step (the step the head took is the input of its own Exp_SEK3; what the step should have been
    is returned beside it); break B from the record's own float32 dist, the value the head compared.

    Returns dict(records=[dict(k, ell, ell_max, step, exit_code, dist, borderline_a, next_ell, next_ell_max, dR, dT, R0, T0)],
    n_expected -- how many records the walk wants: up to its first break, at most max_iter --, R, T (float64), ell, ell_max,
    iter, transform, prev_transform, accum_transform (float64), census)."""
    r = rules or RULES
    mode = mode_of(p)
    census = dict.fromkeys(CENSUS_KEYS + CONDITION_KEYS, 0)
    R, T = _f(state0["R"]).reshape(3, 3), _f(state0["T"])
    ell, ell_max = np.float32(state0["ell"]), np.float32(state0["ell_max"])
    if mode == "acvo":   # set_pcd's tail, adaptive_cvo.cpp:476-477 (ell_max: the library's parameter for the reference's 0.15)
        ell, ell_max = np.float32(p.ell_init), np.float32(p.ell_max_init)
    used = np.asarray(state0["transform"], np.float64)
    records, break_k, had_root = [], None, False
    for k, t in enumerate(trace[:max(int(p.max_iter), 0)]):
        used = tf_of(R, T)
        rec = dict(k=k, ell=ell, ell_max=ell_max, R0=R, T0=T)
        want = r.step(t["bcde"], p.min_step)
        rec["step"] = want
        if want is None:
            census["step_skipped"] += 1
        else:
            pos = positive_roots(t["bcde"])
            census["step_min_late"] += bool(had_root and not pos)   # (min_step after steps from a root)
            had_root = had_root or bool(pos)
            census["step_min" if not pos else ("step_clamped" if want == float(STEP_MAX) else "step_unclamped")] += 1
        stop = r.stops_on_twist(mode, t["omega"], t["v"], p.eps)[0]
        border = stops_on_twist(mode, t["omega"], t["v"], p.eps)[1]   # (a condition on the case: judged by this module's rule, whatever `rules`)
        rec["borderline_a"] = border
        census["borderline_a"] += bool(border)
        code = 0
        rec["dist"], rec["dR"], rec["dT"] = np.nan, None, None
        if stop:
            code = 1
        else:
            census["borderline_theta"] += bool(theta32(t["omega"])[1])
            census["small_angle"] += bool(small_angle(t["omega"]))
            dR, dT = r.exp_sek3(t["omega"], t["v"], t["step"])
            R, T = r.update(R, T, dR, dT)
            rec["dR"], rec["dT"] = dR, dT
            rec["dist"] = r.dist(*r.dist_arguments(dR, dT, R, T))
            if np.float32(t["dist"]) < np.float32(p.eps_2):
                code = 2
        rec["exit_code"] = code
        n_ell, n_max = r.ell_after(r, mode, k, ell, ell_max, t["dl"], p, code)
        if code == 0:
            if mode == "acvo":
                raw = np.float32(float(ell) + float(p.dl_step) * float(t["dl"]))
                census["shrink"] += bool(raw >= ell_max)
                census["floor"] += bool((np.float32(float(ell_max) * 0.7) if raw >= ell_max else raw) < np.float32(p.ell_min))
            else:
                for at in (3, 10, 20):
                    census["schedule_%d" % at] += (k == at and n_ell != ell)
        rec["next_ell"], rec["next_ell_max"] = n_ell, n_max
        ell, ell_max = n_ell, n_max
        records.append(rec)
        if code:
            break_k = k
            census["break_a" if code == 1 else "break_b"] += 1
            break
    if break_k is None:
        census["max_iter"] += 1
    tf, prev, accum = r.finish(state0, used, R, T)
    n_expected = len(records) if break_k is not None else max(int(p.max_iter), 0)
    return dict(records=records, n_expected=n_expected, R=R, T=T, ell=ell, ell_max=ell_max,
                iter=r.final_iter(int(state0["iter"]), break_k, int(p.max_iter)), transform=tf, prev_transform=prev,
                accum_transform=accum, census=census)


def positive_roots(bcde):
    """The positive real roots roots_step chose among (none for a degenerate cubic): for the census and the mutants."""
    found = cubic_roots(bcde)
    return [] if found is None else list(found[0])
