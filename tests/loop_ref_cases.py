"""What tests/test_loop_ref_cpu.py and tests/test_gpu_loop_ref.py share: the settings, the runs, the tolerances that hold
a float32 head (the oracle's, the library's) to the float64 replay of tests/cvo_loop_ref.py, the judge that applies them,
and the mutants.  A plain module; no test lives here.

Exact parts (no tolerance): k, exit_code, every ell and ell_max, iter, omega == (float)omega_d, v == (float)v_d, break B on
the record's own float32 dist, prev_transform against the transform of the run one iteration shorter.
Figures the project already uses: the step within 1e-5 relative of numpy.roots (tests/test_host_math.py,
tests/test_gpu_iteration_ref.py); dist within 2e-5 relative + 1e-7 of logm (test_dist_se3_matches_matrix_log).
Break A: a record whose norm lies within cvo_loop_ref.A_BAND_CVO (3 u: a float32 norm is three squares and two additions --
3 u of the sum of squares --, halved by the root, plus the root's own rounding: 2.5 u) or A_BAND_ACVO (1e-12) of eps is
borderline; so is a record whose |omega| lies within 3 u of Exp_SEK3's TOLERANCE.  A condition on the cases: there is none,
and no record's cubic has a nearly double root.

One update of the pose (update_tol), u = 2^-24, to first order in u, by the method of tests/iteration_ref_cases.py (K
roundings times the absolute-value majorant).  Exp_SEK3 as LieGroup.cpp:172-179 writes it in float, phi = dt theta:
    theta = |omega|                      3 u relative;   theta2 = theta theta  7 u;   theta2 theta  11 u
    A = skew(omega) exact;  A2 = A A     three products, two additions: 3 u (|A||A|)
    fl(dt theta)                         4 u phi; sin of it: 4 u phi |cos| + 2 u |sin| (a libm within an ulp) <= 6 u phi
                                         cos of it: 4 u phi |sin| + 2 u |cos| <= 4 u phi^2 + 2 u
    c1 = stheta / theta                  (6 + 3 + 1) u dt = 10 u dt         -- relative to phi / theta = dt, not to sin / theta
    c2 = (1 - ctheta) / theta2           the difference: 2 u + 4 u phi^2 + u (1 - cos phi) ABSOLUTE -- the cancellation at small
                                         phi is relative to 1, not to the difference -- over theta2, and (7 + 1) u of c2:
                                         e2 = u (2 + 4 phi^2 + 9 (1 - cos phi)) / theta^2
    c3 = (dt theta - stheta) / theta^3   the difference: 4 u phi + 6 u phi + u (phi - sin phi) absolute -- relative to phi --
                                         over theta^3, and (11 + 1) u of c3:  e3 = u (10 phi + 13 (phi - sin phi)) / theta^3
    R  = (I + c1 A) + c2 A2              10 u dt |A| + u c1 |A|;  e2 (|A||A|) + 4 u c2 (|A||A|);  two additions: 2 u of the
                                         absolute sum I + c1 |A| + c2 (|A||A|)
    Jl = (dt I + c2 A) + c3 A2           e2 |A| + u c2 |A|;  e3 (|A||A|) + 4 u |c3| (|A||A|);  2 u (dt I + c2 |A| + |c3| (|A||A|))
    dT = Jl v                            tol(Jl) |v| + 3 u |Jl| |v|
  (entries of A A are at most theta^2, so e2 (|A||A|) <= 2 u + ... and e3 (|A||A|) |v| <= 10 u dt |v| + ...: both stay of order u.)
  The small-angle branch: dR = I, dT = v, exact.
The update (cvo.cpp:398-399): R dT + T: |R| tol(dT) + 3 u |R||dT| + u (|R||dT| + |T|);  R dR: |R| tol(dR) + 3 u |R||dR|.
With |theta| dt of 1e-3 ... 0.5 and |R| <= 1 this is 5e-7 ... 2e-6 per entry.

The pose after a whole registration of n updates (no run one shorter to start from): the single-update bounds add up; an
error already in R is rotated by the later updates, which can move sqrt(3) of its largest entry into one entry, and enters
T through R dT: tol(R) = sqrt(3) sum_i max tol_i(R), tol(T) = sum_i (max tol_i(T) + 3 tol_i-1(R) max|dT_i|).  Looser by
construction: it catches drift and bookkeeping, not order errors.

transform = [R' | -R' T] of the state's own float32 R, T: R' exact, -R' T three products and two additions: 3 u |R'||T|.
accum_transform = accum prev (cvo.cpp:414), four products and three additions per entry: 4 u |accum||prev|.

A min_step step at k > 0, after steps from a root: a bounded search on the CPU (c, d from 1e-3 to 1e5, the moving cloud
shifted by 0 ... 0.45 m, both modes) found valid settings -- where the clouds overlap only in their kernels' tails, A is not
empty at ell = 0.15 and empties when the schedule lowers ell: cvo's defaults with the moving cloud shifted by 0.2 m have
121 members at k = 0 and none from k = 21 on (ell = 0.03).  It is the setting cvo_empties_at_21, census key step_min_late.

The mutants.  Each restates one function of cvo_loop_ref with one plausible error of a head; the CPU file holds that the
judge fails each on some run by something a head with that error would produce -- a verdict, an exit code, a value; the
conditions on the cases (borderline records, skipped steps) are always judged by cvo_loop_ref's own rule and reject
nothing.  Float norms in acvo's break A are told apart by acvo_eps_on_a_norm, whose eps is made from the registration's own
trace (eps_on_a_norm): the double norm breaks, a float norm does not.  One mutant is out of reach by construction and is
listed apart (UNREACHABLE_MUTANTS; the CPU file holds that it survives): double norms in cvo's break A differ from float
norms only where the norm lies within the float norm's own rounding of eps, and there the reference's text does not decide
either (the order of Eigen's three additions and a fused multiply-add are the compiler's): the judge calls such a record
borderline and the cases must hold none.
"""
import numpy as np

import cvo_loop_ref as lr
import iteration_ref_cases as ic

U = lr.U
STEP_REL = 1e-5
DIST_REL, DIST_ABS = 2e-5, 1e-7
SIZES = [(300, 260), (260, 300)]
PREFIX_J = dict(cvo=6, acvo=4)
THIRD_FRAME_SHIFT = np.array([0.01, -0.005, 0.008])

EPS_CASE = "acvo_eps_on_a_norm"
# (name, mode, parameter overrides, shift of the moving cloud in metres)
SETTINGS = [
    ("cvo_default", "cvo", dict(max_iter=40), 0.0),
    ("acvo_default", "acvo", dict(), 0.0),
    ("matlab", "matlab", dict(), 0.0),
    ("cvo_cd_small", "cvo", dict(c=0.07, d=0.07, max_iter=40), 0.0),
    ("cvo_cd_large", "cvo", dict(c=700.0, d=700.0, max_iter=40), 0.0),
    ("cvo_break_b", "cvo", dict(eps_2=1e-2, max_iter=40), 0.0),
    ("cvo_break_b_at_3", "cvo", dict(eps_2=2.5e-3, max_iter=40), 0.0),      # (a break where the schedule would change ell)
    ("cvo_break_a_at_0", "cvo", dict(eps=0.5, max_iter=40), 0.0),
    ("cvo_far_min_step_0.2", "cvo", dict(min_step=0.2, max_iter=5), 10.0),
    ("cvo_far_min_step_0.05", "cvo", dict(min_step=0.05, max_iter=5), 10.0),
    ("cvo_far_min_step_1.5", "cvo", dict(min_step=1.5, max_iter=5), 10.0),
    ("cvo_empties_at_21", "cvo", dict(max_iter=25), 0.2),                     # (121 members at k = 0, none at ell = 0.03)
    ("cvo_small_angle", "cvo", dict(c=1e9, max_iter=40), 0.0),
    ("acvo_small_angle", "acvo", dict(c=1e9, d=0.5, max_iter=40), 0.0),
    ("acvo_shrink", "acvo", dict(ell_max_init=0.101, dl_step=-0.3, max_iter=40), 0.0),
    ("acvo_shrink_fast", "acvo", dict(ell_max_init=0.2, dl_step=-30.0, max_iter=40), 0.0),
    ("acvo_ell_meets_ell_max", "acvo", dict(dl_step=0.0, ell_max_init=0.1, max_iter=8), 0.0),   # (ell == ell_max: the >= of :541)
    ("acvo_floor", "acvo", dict(dl_step=3.0, max_iter=40), 0.0),
    # eps is set from the registration's OWN trace (eps_on_a_norm): the float32 that a record's larger norm rounds UP to.  The
    # double norm is below it and breaks; a float norm equals it and does not
    (EPS_CASE, "acvo", dict(), 0.0),
    ("cvo_long_walk", "cvo", dict(eps=0.0, eps_2=0.0, max_iter=150), 0.0),
]
PREFIX_SETTINGS = ("cvo_default", "acvo_default")


def setting(name):
    return next(s for s in SETTINGS if s[0] == name)


def params(api, mode, over):
    p = api.default_params(ic.mode_id(api, mode))
    for key, value in over.items():
        setattr(p, key, value)
    return p


def clouds(pkg, mode, n, m, shift=0.0):
    xf, ff, xm, fm = ic.clouds(pkg, mode, n, m)
    if shift:
        xm = (xm.astype(np.float64) + shift).astype(np.float32)
    return xf, ff, xm, fm


def third_frame(xm):
    return (xm.astype(np.float64) + THIRD_FRAME_SHIFT).astype(np.float32)


def snap(s):
    """A state struct (the oracle's and the library's have one layout) as float32 arrays."""
    f = np.float32
    return dict(R=np.array(s.R, f).reshape(3, 3), T=np.array(s.T, f), ell=f(s.ell), ell_max=f(s.ell_max), iter=int(s.iter),
                transform=np.array(s.transform, f).reshape(4, 4), prev_transform=np.array(s.prev_transform, f).reshape(4, 4),
                accum_transform=np.array(s.accum_transform, f).reshape(4, 4))


def same_state(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def same_records(a, b):
    """Two traces' records, bit for bit in everything the head wrote (dist is NaN where break A fired)."""
    keys = ("k", "exit_code", "ell", "step", "dist", "omega", "v")
    return len(a) == len(b) and all(np.array_equal(np.array(x[k], np.float32), np.array(y[k], np.float32), equal_nan=True)
                                    for x, y in zip(a, b) for k in keys)


# ---- tolerances

def exp_tol(omega, v, dt):
    """(tol dR (3, 3), tol dT (3,)) of Exp_SEK3 in float32 (module docstring)."""
    w, vv, dt = lr._f(omega), lr._f(v), float(np.float32(dt))
    if lr.small_angle(omega):
        return np.zeros((3, 3)), np.zeros(3)
    th = float(np.sqrt(w @ w))
    phi = dt * th
    A = np.abs(lr.skew(w))
    AA = A @ A
    c1, c2, c3 = np.sin(phi) / th, (1.0 - np.cos(phi)) / th ** 2, (phi - np.sin(phi)) / th ** 3
    e1 = 10.0 * U * dt
    e2 = U * (2.0 + 4.0 * phi ** 2 + 9.0 * (1.0 - np.cos(phi))) / th ** 2
    e3 = U * (10.0 * phi + 13.0 * (phi - np.sin(phi))) / th ** 3
    eye = np.eye(3)
    tol_r = e1 * A + U * abs(c1) * A + e2 * AA + 4.0 * U * c2 * AA + 2.0 * U * (eye + abs(c1) * A + c2 * AA)
    jl_abs = dt * eye + c2 * A + abs(c3) * AA
    tol_jl = e2 * A + U * c2 * A + e3 * AA + 4.0 * U * abs(c3) * AA + 2.0 * U * jl_abs
    return tol_r, tol_jl @ np.abs(vv) + 3.0 * U * (jl_abs @ np.abs(vv))


def update_tol(R, T, omega, v, dt, dR, dT):
    """(tol R, tol T) of one update from the exact float32 state R, T (module docstring)."""
    tol_dr, tol_dt = exp_tol(omega, v, dt)
    aR = np.abs(R)
    return aR @ tol_dr + 3.0 * U * (aR @ np.abs(dR)), aR @ tol_dt + 4.0 * U * (aR @ np.abs(dT)) + U * np.abs(T)


def walk_tol(records, trace):
    """(tol R, tol T): scalars for the pose after all the updates of a replay (module docstring)."""
    acc_r = acc_t = 0.0
    for rec, t in zip(records, trace):
        if rec["dR"] is None:
            continue
        tr, tt = update_tol(rec["R0"], rec["T0"], t["omega"], t["v"], t["step"], rec["dR"], rec["dT"])
        acc_t += float(tt.max()) + 3.0 * acc_r * float(np.abs(rec["dT"]).max())
        acc_r += np.sqrt(3.0) * float(tr.max())
    return acc_r, acc_t


class Worst(dict):
    """The worst error / tolerance ratio seen per quantity, and the worst absolute error."""
    def see(self, key, err, tol):
        err, tol = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(tol, np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / tol)   # (an exact entry, tolerance 0: 0 where it is met)
        a = self.setdefault(key, [0.0, 0.0])
        a[0], a[1] = max(a[0], float(np.max(ratio))), max(a[1], float(np.max(err)))


# ---- the judge

def judge(p, state0, trace, n_it, state1, rules=None, shorter=None, worst=None, census=None):
    """Everything one align() -- its trace, the iterations it reports, the state before and after -- must satisfy under the
    replay with `rules`; the failures as a list of strings (empty: it passes).  shorter: (state, trace, n_it) of the same
    registration with max_iter one less: the run must extend it bit for bit, the pose is then held one update at a time and
    prev_transform bit for bit; without it the pose is held to the walk's bound.  worst / census: accumulators."""
    rules = rules or lr.RULES
    worst = worst if worst is not None else Worst()
    bad = []
    rp = lr.replay(p, state0, trace, rules)
    if census is not None:
        for k, c in rp["census"].items():
            census[k] = census.get(k, 0) + c
    for k in lr.CONDITION_KEYS:
        if rp["census"][k]:
            bad.append("condition: %s in %d records" % (k, rp["census"][k]))
    if not (n_it == len(trace) == rp["n_expected"]):
        bad.append("iterations: reported %d, records %d, the replay wants %d" % (n_it, len(trace), rp["n_expected"]))
    f32 = np.float32
    for rec, t in zip(rp["records"], trace):
        k = rec["k"]
        if t["k"] != k:
            bad.append("k: record %d says %d" % (k, t["k"]))
        if f32(t["ell"]) != rec["ell"]:
            bad.append("ell: record %d has %r, the replay %r" % (k, f32(t["ell"]), rec["ell"]))
        if not (np.array_equal(np.array(t["omega"], f32), np.array(t["omega_d"], np.float64).astype(f32)) and
                np.array_equal(np.array(t["v"], f32), np.array(t["v_d"], np.float64).astype(f32))):
            bad.append("twist: record %d is not its float64 sums cast to float" % k)
        if rec["step"] is not None:
            err = abs(float(t["step"]) - rec["step"])
            worst.see("step", err, STEP_REL * abs(rec["step"]))
            if not err <= STEP_REL * abs(rec["step"]):
                bad.append("step: record %d took %r, the replay wants %r" % (k, t["step"], rec["step"]))
        if t["exit_code"] != rec["exit_code"]:
            bad.append("exit_code: record %d has %d, the replay %d" % (k, t["exit_code"], rec["exit_code"]))
        if rec["exit_code"] == 1:
            if not np.isnan(t["dist"]):
                bad.append("dist: record %d broke on the twist and carries a dist" % k)
        else:
            err, tol = abs(float(t["dist"]) - rec["dist"]), DIST_REL * abs(rec["dist"]) + DIST_ABS
            worst.see("dist", err, tol)
            worst.see("dist_rel", err / abs(rec["dist"]) if rec["dist"] else 0.0, DIST_REL)
            if not err <= tol:
                bad.append("dist: record %d has %r, the replay %r" % (k, t["dist"], rec["dist"]))
    # the state afterwards: the exact parts
    for key in ("ell", "ell_max", "iter"):
        if state1[key] != rp[key]:
            bad.append("%s: the state has %r, the replay %r" % (key, state1[key], rp[key]))
    R1, T1 = state1["R"].astype(np.float64), state1["T"].astype(np.float64)
    used = None
    if shorter is not None:
        s_state, s_trace, s_n = shorter
        if not (s_n == n_it - 1 and lr_prefix(s_trace, trace)):
            bad.append("prefix: the run one iteration shorter is not a prefix of this one")
        elif rp["records"] and rp["records"][-1]["dR"] is not None:
            t = trace[-1]
            R0, T0 = s_state["R"].astype(np.float64), s_state["T"].astype(np.float64)
            dR, dT = rules.exp_sek3(t["omega"], t["v"], t["step"])
            Rw, Tw = rules.update(R0, T0, dR, dT)
            tol_r, tol_t = update_tol(R0, T0, t["omega"], t["v"], t["step"], dR, dT)
            worst.see("update_R", np.abs(R1 - Rw), tol_r)
            worst.see("update_T", np.abs(T1 - Tw), tol_t)
            if not (np.all(np.abs(R1 - Rw) <= tol_r) and np.all(np.abs(T1 - Tw) <= tol_t)):
                bad.append("update: R off by %.3g (bound %.3g), T by %.3g (bound %.3g)"
                           % (np.abs(R1 - Rw).max(), tol_r.max(), np.abs(T1 - Tw).max(), tol_t.max()))
        elif not (np.array_equal(state1["R"], s_state["R"]) and np.array_equal(state1["T"], s_state["T"])):
            bad.append("update: the last record made none and the pose changed")
        used = s_state["transform"]
    else:
        tol_r, tol_t = walk_tol(rp["records"], trace)
        worst.see("walk_R", np.abs(R1 - rp["R"]), tol_r)
        worst.see("walk_T", np.abs(T1 - rp["T"]), tol_t)
        if not (np.all(np.abs(R1 - rp["R"]) <= tol_r) and np.all(np.abs(T1 - rp["T"]) <= tol_t)):
            bad.append("walk: after %d records R off by %.3g (bound %.3g), T by %.3g (bound %.3g)"
                       % (len(trace), np.abs(R1 - rp["R"]).max(), tol_r, np.abs(T1 - rp["T"]).max(), tol_t))
    # the three matrices
    want_tf = lr.tf_of(R1, T1)
    tol_tf = np.zeros((4, 4))
    tol_tf[:3, 3] = 3.0 * U * (np.abs(R1.T) @ np.abs(T1))
    worst.see("transform", np.abs(state1["transform"] - want_tf), tol_tf)
    if not np.all(np.abs(state1["transform"] - want_tf) <= tol_tf):
        bad.append("transform: not [R' | -R' T] of the state's own R, T")
    if not rp["records"]:
        used = state0["transform"]
        if not np.array_equal(state1["transform"], state0["transform"]):
            bad.append("transform: no iteration ran and the transform changed")
    if used is not None:
        _, prev_w, accum_w = rules.finish(state0, used, R1, T1)
        if not np.array_equal(state1["prev_transform"].astype(np.float64), prev_w):
            bad.append("prev_transform: not the transform of the top of the last executed iteration, bit for bit")
        tol_acc = 4.0 * U * (np.abs(state0["accum_transform"].astype(np.float64)) @ np.abs(prev_w))
    else:
        # (no run one shorter: the transform in use comes from the replay's own pose, the walk's bound on it)
        _, prev_w, accum_w = rules.finish(state0, rp["prev_transform"], rp["R"], rp["T"])
        tol_r, tol_t = walk_tol(rp["records"][:-1], trace)
        tol_prev = np.full((4, 4), tol_r)   # (R' is a copy of R; -R' T: the errors of R and T and its own three roundings)
        tol_prev[:3, 3] = 3.0 * tol_r * np.abs(rp["T"]).max() + np.sqrt(3.0) * tol_t + 3.0 * U * np.sqrt(3.0) * max(np.abs(rp["T"]).max(), 1e-30)
        tol_prev[3, :] = 0.0
        worst.see("prev_transform", np.abs(state1["prev_transform"] - prev_w), tol_prev)
        if not np.all(np.abs(state1["prev_transform"] - prev_w) <= tol_prev):
            bad.append("prev_transform: off by %.3g" % np.abs(state1["prev_transform"] - prev_w).max())
        a0 = np.abs(state0["accum_transform"].astype(np.float64))
        tol_acc = 4.0 * U * (a0 @ np.abs(prev_w)) + a0 @ tol_prev
    worst.see("accum_transform", np.abs(state1["accum_transform"] - accum_w), tol_acc)
    if not np.all(np.abs(state1["accum_transform"] - accum_w) <= tol_acc):
        bad.append("accum_transform: off by %.3g" % np.abs(state1["accum_transform"] - accum_w).max())
    return bad


def lr_prefix(short, full):
    return len(short) + 1 == len(full) and same_records(short, full[:len(short)])


# ---- the runs.  `driver(api, ps, mode, frames)` is the oracle's or the library's: it registers frames[i + 1] (moving) to
# frames[i] (fixed) with parameters ps[i], all on ONE state, and returns [(n_it, trace, state before, state after)].

def run_frames(api, driver, mode, ps, frames, name, size):
    out = driver(api, ps, mode, frames)
    return [dict(name=name, size=size, p=p, n_it=n, trace=tr, state0=s0, state1=s1) for p, (n, tr, s0, s1) in zip(ps, out)]


def run_setting(api, driver, pkg, name, size, max_iter=None):
    """One registration of a setting from a fresh state: dict(name, size, p, state0, trace, n_it, state1)."""
    _, mode, over, shift = setting(name)
    p = params(api, mode, over)
    if max_iter is not None:
        p.max_iter = max_iter
    xf, ff, xm, fm = clouds(pkg, mode, size[0], size[1], shift)
    if name == EPS_CASE:   # (two registrations: the first one's trace says where eps goes)
        p.eps = eps_on_a_norm(run_frames(api, driver, mode, [p], [(xf, ff), (xm, fm)], name, size)[0]["trace"])
    return run_frames(api, driver, mode, [p], [(xf, ff), (xm, fm)], name, size)[0]


def eps_on_a_norm(trace, first=5):
    """An eps that makes break A depend on the precision of the norm, from a registration's own trace: the first record k >=
    `first` whose larger norm n rounds UP to its nearest float32 f (f > n, by half an ulp at most: 6e-8, far outside acvo's
    1e-12 band), while no earlier record has both norms below f.  With eps = f the double norms of adaptive_cvo.cpp:509 break
    at k (n < f); a correctly rounded float norm is f itself and does not."""
    norms = [(float(np.sqrt(np.sum(lr._f(t["omega"]) ** 2))), float(np.sqrt(np.sum(lr._f(t["v"]) ** 2)))) for t in trace]
    for k in range(first, len(norms)):
        n = max(norms[k])
        f = float(np.float32(n))
        if f > n and (f - n) > 1e-10 * n and not any(max(a) < f for a in norms[:k]):
            return f
    raise AssertionError("no record's norm rounds up: the case cannot be made from this trace")


def run_prefixes(api, driver, pkg, name, size):
    """The same registration with max_iter = 0, 1 ... J."""
    mode = setting(name)[1]
    return [run_setting(api, driver, pkg, name, size, max_iter=j) for j in range(PREFIX_J[mode] + 1)]


def run_carry_over(api, driver, pkg, mode, size):
    """Three frames on one state -- the pair, then the moving cloud shifted as a third frame -- and a fourth registration
    with max_iter = 0 on the state they leave."""
    xf, ff, xm, fm = clouds(pkg, mode, size[0], size[1])
    ps = [params(api, mode, dict(max_iter=40)), params(api, mode, dict(max_iter=40)), params(api, mode, dict(max_iter=0))]
    frames = [(xf, ff), (xm, fm), (third_frame(xm), fm), (xf, ff)]
    return run_frames(api, driver, mode, ps, frames, "carry_over_" + mode, size)


def judge_run(run, rules=None, shorter=None, worst=None, census=None):
    sh = (shorter["state1"], shorter["trace"], shorter["n_it"]) if shorter is not None else None
    return judge(run["p"], run["state0"], run["trace"], run["n_it"], run["state1"], rules=rules, shorter=sh, worst=worst,
                 census=census)


# ---- the mutants: cvo_loop_ref with one plausible error of a head each

def _m_update_r_first(R, T, dR, dT):
    Rn = R @ dR
    return Rn, Rn @ dT + T


def _m_update_left(R, T, dR, dT):
    return dR @ R, R @ dT + T


def _m_exp_scaled_small(omega, v, dt):
    if lr.small_angle(omega):
        return np.eye(3), float(np.float32(dt)) * lr._f(v)
    return lr.exp_sek3(omega, v, dt)


def _m_stops_float_in_acvo(mode, omega, v, eps):
    """float norms in acvo's break A (correctly rounded ones: the float32 nearest to the norm)"""
    if mode != "acvo":
        return lr.stops_on_twist(mode, omega, v, eps)
    nw, nv = (np.float32(np.sqrt(np.sum(lr._f(x) ** 2))) for x in (omega, v))
    return bool(nw < np.float32(eps) and nv < np.float32(eps)), False


def _m_stops_double_in_cvo(mode, omega, v, eps):
    """double norms in cvo's break A: the verdict of the double comparison, whatever the band"""
    return lr.stops_on_twist(mode, omega, v, eps)[0], False


def _m_ell_gt(mode, k, ell, ell_max, dl, p):
    if mode != "acvo":
        return lr.next_ell(mode, k, ell, ell_max, dl, p)
    ell, ell_max = np.float32(ell), np.float32(ell_max)
    ell = np.float32(float(ell) + float(p.dl_step) * float(dl))
    if ell > ell_max:
        ell = ell_max = np.float32(float(ell_max) * 0.7)
    return (np.float32(p.ell_min) if ell < np.float32(p.ell_min) else ell), ell_max


def _m_ell_max_from_new(mode, k, ell, ell_max, dl, p):
    if mode != "acvo":
        return lr.next_ell(mode, k, ell, ell_max, dl, p)
    ell, ell_max = np.float32(ell), np.float32(ell_max)
    ell = np.float32(float(ell) + float(p.dl_step) * float(dl))
    if ell >= ell_max:
        ell = np.float32(float(ell_max) * 0.7)
        ell_max = np.float32(float(ell) * 0.7)
    return (np.float32(p.ell_min) if ell < np.float32(p.ell_min) else ell), ell_max


def _m_floor_first(mode, k, ell, ell_max, dl, p):
    if mode != "acvo":
        return lr.next_ell(mode, k, ell, ell_max, dl, p)
    ell, ell_max = np.float32(ell), np.float32(ell_max)
    ell = np.float32(float(ell) + float(p.dl_step) * float(dl))
    if ell < np.float32(p.ell_min):
        ell = np.float32(p.ell_min)
    if ell >= ell_max:
        ell = ell_max = np.float32(float(ell_max) * 0.7)
    return ell, ell_max


def _m_schedule_off_by_one(mode, k, ell, ell_max, dl, p):
    return lr.next_ell(mode, k + 1 if mode != "acvo" else k, ell, ell_max, dl, p)


def _m_ell_on_break(rules, mode, k, ell, ell_max, dl, p, exit_code):
    return rules.next_ell(mode, k, ell, ell_max, dl, p)


def _m_finish_final(state0, used_transform, R, T):
    tf = lr.tf_of(R, T)
    return tf, np.asarray(used_transform, np.float64), np.asarray(state0["accum_transform"], np.float64) @ tf.astype(np.float32)


def _m_iter_max(iter0, break_k, max_iter):
    return max_iter if break_k is None else break_k


def _m_min_step_unclamped(bcde, min_step):
    want = lr.step(bcde, min_step)
    if want is not None and not lr.positive_roots(bcde):
        return float(np.float32(min_step))
    return want


def _m_largest_root(bcde, min_step):
    pos = lr.positive_roots(bcde)
    if lr.step(bcde, min_step) is None or not pos:
        return lr.step(bcde, min_step)
    return float(min(np.float32(max(pos)), lr.STEP_MAX))


MUTANTS = {
    "R updated before T": lr.with_rule(update=_m_update_r_first),
    "dR R instead of R dR": lr.with_rule(update=_m_update_left),
    "dT scaled by the step in the small-angle branch": lr.with_rule(exp_sek3=_m_exp_scaled_small),
    "float norms in acvo's break A": lr.with_rule(stops_on_twist=_m_stops_float_in_acvo),
    "ell > ell_max instead of >=": lr.with_rule(next_ell=_m_ell_gt),
    "ell_max shrunk from the new ell": lr.with_rule(next_ell=_m_ell_max_from_new),
    "the floor applied before the shrink": lr.with_rule(next_ell=_m_floor_first),
    "the cvo schedule in force from iteration 3 on (applied after k = 2)": lr.with_rule(next_ell=_m_schedule_off_by_one),
    "the schedule applied in the iteration that breaks": lr.with_rule(ell_after=_m_ell_on_break),
    "accum_transform multiplied by the final transform": lr.with_rule(finish=_m_finish_final),
    "iter = max_iter at the max_iter stop": lr.with_rule(final_iter=_m_iter_max),
    "min_step not clamped": lr.with_rule(step=_m_min_step_unclamped),
    "the largest positive root": lr.with_rule(step=_m_largest_root),
    "dist of (R, T) instead of (dR, dT)": lr.with_rule(dist_arguments=lambda dR, dT, R, T: (R, T)),
}
# Out of reach by construction (module docstring): the judge must NOT tell it apart on cases without a borderline record.
UNREACHABLE_MUTANTS = {
    "double norms in cvo's break A": lr.with_rule(stops_on_twist=_m_stops_double_in_cvo),
}
