"""What tests/test_pair_weight_cpu.py and tests/test_gpu_pair_weight.py share: parameter sets far from the shipped
constants, the inputs they run on, and the rule that keeps borderline pairs out of the comparison with the float64
reference.  A plain module; no test lives here.

Why.  At the shipped constants the pair weight (csrc/cvo_pair.h, oracle/cvo_oracle.c pair_weight) sees exponents in
(-0.22, 0] (spatial) and (-4.83, 0] (colour), and two of its three cuts never decide (iteration_ref_cases.ACVO_VARIANTS).
cvo_hip_set_params admits any positive finite kernel scale and threshold.  The sets below take the exponents to 83, let
each cut decide, and visit the edges: thresholds at and above sigma^2 (no member), weights below FLT_MIN.

The star.  K = 2400 fixed points on a cubic grid whose spacing is four radii sqrt(tau) of the set at the length scale plus
1 m, centred on the origin; fixed point j has ONE partner, moving point j, so that every member is a pair (j, j) and
cvo_hip_pose_matches' best_w[j] is the float32 weight of that pair as bits.  Three groups by j mod 24:
    j mod 24 < 10   "spatial":  d2 uniform in [0, 1.05 tau],       d2c uniform in [0, 0.02 tau_c']
    j mod 24 < 20   "colour":   d2 uniform in [0, 0.02 tau],       d2c uniform in [0, 1.05 tau_c']
    else            "both":     d2 uniform in [0, 1.05 tau],       d2c uniform in [0, 1.05 tau_c']
tau_c' = 2 c_l^2 min(ln(cs2 / c_sp), ln(s2 cs2 / sp)): the colour cut's own tau_c where that cut can decide, and the
colour distance at which a > sp_thres removes a pair at d2 = 0 where it cannot.  (A pair kept with a colour exponent near
its limit needs a spatial exponent near zero, a > sp being a cut on their sum; with d2 uniform up to 1.05 tau for every
pair, a fifteenth of them would be kept past 40 on either exponent in cvo_far_both.  Hence the groups.)  The MATLAB weight
has no colour cut: d2 is uniform in [0, 1.05 tau] for every pair there.  A set without members is drawn with the mode's
shipped constants: at those, the pairs would be members.
Features: a base in [1, 100]^5 (acvo: [0.01, 0.5]^5) and the partner's at the drawn distance in a direction with
non-negative components, so that every feature is positive (the MATLAB weight's KW needs non-negative colours, and a black
point has no member).
Poses: the identity and iteration_ref_cases.small_motion(); the moving cloud is R y + T of the partners y in float64,
rounded, so that po.transform(R, T, xm) lands on the partners to a rounding.  Everything is then judged on the positions
po.transform really gives.

Borderline pairs: |margin| <= cvo_iteration_ref.BAND of cvo_iteration_ref.weights, the rule of
tests/test_iteration_ref_cpu.py.  They are left out of the comparison with the float64 reference only, never of the
comparison with the oracle.  At most STAR_BORDER_MAX of a star's pairs and DENSE_BORDER_MAX of a dense pair's candidates
may be borderline; star() and dense_case() assert it.
"""
import functools

import numpy as np

import cvo_iteration_ref as ref
import iteration_ref_cases as ic

K_STAR = 2400
GRID = 14                      # 14^3 = 2744 >= K_STAR grid nodes
STAR_BORDER_MAX = 8
DENSE_BORDER_MAX = 1e-3        # of the candidates N * M
DENSE_SIZES = [(300, 260), (257, 63)]
FLT_MIN = float(np.finfo(np.float32).tiny)


def _s2(p):
    return np.float32(p.sigma) * np.float32(p.sigma)


def _cs2(p):
    return np.float32(p.c_sigma) * np.float32(p.c_sigma)


def _no_colour_threshold(p):
    """The smallest float32 c_sp >= c_sigma^2 whose quotient c_sp / c_sigma / c_sigma, formed in float32 as the library and
    the oracle form it, is not below 1: log of it is >= 0 and tau_c <= 0."""
    cs = np.float32(p.c_sigma)
    t = np.float32(cs * cs)
    while np.float32(np.float32(t / cs) / cs) < np.float32(1.0):
        t = np.nextafter(t, np.float32(np.inf))
    return float(t)


class Set:
    def __init__(self, name, mode, over, ells, point, members=True):
        self.name, self.mode, self.over, self.ells, self.point, self.members = name, mode, over, ells, point, members
        self.fusable = mode != "matlab"   # (the MATLAB weight stays out of the engines by design)

    def __repr__(self):
        return self.name

    def params(self, api):
        """default_params of the mode with the set's overrides, for api = the oracle's or the library's Python face."""
        p = api.default_params(ic.mode_id(api, self.mode))
        for key, value in self.over.items():
            setattr(p, key, value(p) if callable(value) else value)
        return p


# cvo_colour_cut.  In cvo the colour cut is ck > sp_thres and a > sp_thres is ck > sp_thres / k with k <= sigma^2: at the
# shipped sigma = 0.1 (s2 = 0.01) the latter is a hundred times tighter whatever sp_thres and c_ell are, and d2c < tau_c can
# remove nothing of its own.  It decides exactly where k > 1, so the set carries sigma = 2 as well: s2 = 4, and the colour cut
# is the tighter statement for the pairs with d2 / 2 l^2 < ln 4 = 1.39 -- all of the star's "colour" group.  sp_thres = 0.05
# puts tau_c = 2 25 ln 20 = 150 on RGB-scale features (differences of about 12 grey levels) and leaves the radius at
# sqrt(2 ln 80) l = 2.96 l.
# cvo_radius_cut: cs2 = 1.5625, so a > sp is k > sp / ck with ck up to 1.56 and the radius (k > sp) decides where ck > 1.
SETS = [
    Set("cvo_sp1e-6", "cvo", dict(sp_thres=1e-6), (0.15, 0.1, 0.03), "both exponents past 6: the realistic wide kernel"),
    Set("cvo_sp1e-12", "cvo", dict(sp_thres=1e-12), (0.1, 0.04), "spatial exponent to 23"),
    Set("cvo_far_both", "cvo", dict(sp_thres=1e-30, c_ell=60.0), (0.1, 0.04), "both exponents past 40"),
    Set("acvo_sp1e-9", "acvo", dict(sp_thres=1e-9, c_sp_thres=1e-9), (0.1, 0.04), "acvo's two thresholds, HSV-scale features"),
    Set("cvo_wide", "cvo", dict(sigma=1.0, c_sigma=3.0, sp_thres=2e-3), (0.1, 0.04), "s2, cs2 not below 1; ck up to 9"),
    Set("cvo_colour_cut", "cvo", dict(c_ell=5.0, sigma=2.0, sp_thres=0.05), (0.1, 0.04), "d2c < tau_c removes pairs a > sp would keep"),
    Set("cvo_radius_cut", "cvo", dict(c_sigma=1.25), (0.12, 0.07), "d2 < tau decides (the cvo twin of the acvo variant)"),
    Set("matlab_sp1e-8", "matlab", dict(sp_thres=1e-8), (0.1, 0.04), "K >= sp with its >=, 1.00001 on tau, linear colour product"),
    Set("cvo_tight", "cvo", dict(sp_thres=lambda p: float(np.float32(0.9) * _s2(p))), (0.1, 0.04), "a radius of 0.46 l"),
    Set("cvo_subnormal", "cvo", dict(sp_thres=1e-38), (0.1, 0.04), "weights between 1e-38 and FLT_MIN"),
    Set("cvo_no_radius", "cvo", dict(sp_thres=lambda p: float(_s2(p))), (0.1,), "tau = 0: no member", members=False),
    Set("cvo_no_radius_x4", "cvo", dict(sp_thres=lambda p: float(np.float32(4.0) * _s2(p))), (0.1,), "tau < 0: no member", members=False),
    Set("acvo_no_colour", "acvo", dict(c_sp_thres=_no_colour_threshold), (0.1,), "tau_c <= 0: no member", members=False),
]
BY_NAME = {s.name: s for s in SETS}
POSES = ("identity", "small")
# What each set is meant to reach: (which exponent, its magnitude, kept pairs of a star past it at least).  The counts
# follow from the draw: with L = ln(s2 cs2 / sp) the 1000 pairs of the group that carries an exponent E uniform in
# [0, 1.05 L] are kept past a magnitude m where m < E < L, a share (L - m) / 1.05 L of them: 332 (L = 9.2, m = 6),
# 125 (L = 23.0, m = 20) and 362 (L = 64.5, m = 40), a binomial count with a deviation of 10 to 15.  300 where the expected
# count allows it; for cvo_sp1e-12, whose radius ends at 23, two thirds of the expected count.
REACH = {"cvo_sp1e-6": [("E1", 6.0, 300)], "cvo_sp1e-12": [("E1", 20.0, 80)],
         "cvo_far_both": [("E1", 40.0, 300), ("E2", 40.0, 300)]}


def pose(name):
    if name == "identity":
        return np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    return ic.small_motion()


def search_of(po, s):
    return po.SEARCH_DENSE if s.mode == "matlab" else po.SEARCH_GRID


def exponents(p, ell, d2, d2c):
    """(E1, E2): the magnitudes of the two exponents, d2 / 2 l^2 and d2c / 2 c_l^2 (the MATLAB weight has no second)."""
    ell, c_ell = float(np.float32(ell)), float(np.float32(p.c_ell))
    return d2 / (2.0 * ell * ell), (np.zeros_like(d2c) if p.color_scale > 0 else d2c / (2.0 * c_ell * c_ell))


def pair_ref(p, ell, xa, fa, xb, fb):
    """cvo_iteration_ref.weights of the pairs (j, j) alone: (a, d2, d2c, margin), each (K,)."""
    out = [[], [], [], []]
    for k in range(0, len(xa), 64):
        sl = slice(k, k + 64)
        for q, w in zip(out, ref.weights(p, ell, xa[sl], fa[sl], xb[sl], fb[sl], c_sp=ic.c_sp_of(p))):
            q.append(np.diagonal(w).copy())
    return tuple(np.concatenate(q) for q in out)


def _draw_params(po, s):
    return s.params(po) if s.members else po.default_params(ic.mode_id(po, s.mode))


@functools.lru_cache(maxsize=None)
def _star_clouds(po, name, ell, pose_name):
    s = BY_NAME[name]
    q = _draw_params(po, s)
    rng = np.random.default_rng(7000 + 100 * SETS.index(s) + int(round(float(ell) * 1000)))
    tau, tau_c = ref.cuts(q, ell, ic.c_sp_of(q))
    s2, cs2, sp = float(_s2(q)), float(_cs2(q)), float(np.float32(q.sp_thres))
    c_ell = float(np.float32(q.c_ell))
    tau_c = min(tau_c, 2.0 * c_ell * c_ell * np.log(s2 * cs2 / sp))
    assert tau > 0 and tau_c > 0
    j = np.arange(K_STAR)
    u, v = rng.uniform(0.0, 1.05, K_STAR), rng.uniform(0.0, 1.05, K_STAR)
    if s.mode != "matlab":
        u = np.where((j % 24 >= 10) & (j % 24 < 20), u * (0.02 / 1.05), u)
    v = np.where(j % 24 < 10, v * (0.02 / 1.05), v)
    d2, d2c = u * tau, v * tau_c
    spacing = 4.0 * np.sqrt(tau * 1.00001) + 1.0   # (the MATLAB weight's radius carries the factor)
    node = np.stack(np.unravel_index(j, (GRID, GRID, GRID)), 1).astype(np.float64)
    xf = ((node - (GRID - 1) / 2.0) * spacing).astype(np.float32)
    d = rng.normal(size=(K_STAR, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    y = (xf.astype(np.float64) + np.sqrt(d2)[:, None] * d).astype(np.float32)
    R, T = pose(pose_name)
    xm = (y.astype(np.float64) @ R.astype(np.float64).T + T.astype(np.float64)).astype(np.float32)
    lo, hi = (0.01, 0.5) if s.mode == "acvo" else (1.0, 100.0)
    ff = rng.uniform(lo, hi, (K_STAR, 5))
    g = np.abs(rng.normal(size=(K_STAR, 5)))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    fm = ff + np.sqrt(d2c)[:, None] * g
    return xf, ff.astype(np.float32), xm, fm.astype(np.float32), float(spacing)


@functools.lru_cache(maxsize=None)
def star(po, name, ell, pose_name):
    """One star: a dict with the clouds (xf, ff, xm, fm), the pose (R, T), y = po.transform(R, T, xm), the oracle's member
    set (rows, val: every member is (row, row)), the float64 reference of the pairs (j, j) (a, d2, d2c, margin) and its
    classes (sure_in, border, sure_out).  Asserts isolation, row == col and the borderline count."""
    s = BY_NAME[name]
    p = s.params(po)
    xf, ff, xm, fm, spacing = _star_clouds(po, name, ell, pose_name)
    R, T = pose(pose_name)
    y = po.transform(R, T, xm)
    tau = ref.cuts(p, ell, ic.c_sp_of(p))[0] * (1.00001 if s.mode == "matlab" else 1.0)
    reach = np.sqrt(max(tau, 0.0))
    # no point of the other cloud but the partner is within reach: partners are within 1.03 reach of their grid node
    assert np.all(np.linalg.norm(y.astype(np.float64) - xf.astype(np.float64), axis=1) <= 1.03 * reach + 1e-3) or not s.members
    assert spacing >= 4.0 * reach + 1.0 - 1e-9
    rows, cols, val = _members(po, p, ell, xf, ff, y, fm, search_of(po, s))
    assert np.array_equal(rows, cols), (name, ell, pose_name)
    a, d2, d2c, margin = pair_ref(p, ell, xf, ff, y, fm)
    sure_in, border, sure_out = ref.classify(margin)
    assert int(border.sum()) <= STAR_BORDER_MAX, (name, ell, pose_name, int(border.sum()))
    return dict(set=s, p=p, ell=ell, pose=pose_name, R=R, T=T, xf=xf, ff=ff, xm=xm, fm=fm, y=y, rows=rows, val=val,
                a=a, d2=d2, d2c=d2c, margin=margin, sure_in=sure_in, border=border, sure_out=sure_out)


def _members(po, p, ell, xa, fa, xb, fb, search):
    rp, col, val = po.se_kernel(p, ell, xa, fa, xb, fb, search=search)
    return np.repeat(np.arange(len(xa)), np.diff(rp)), col, val


def star_cases():
    """(set name, ell, pose name) of every star."""
    return [(s.name, ell, ps) for s in SETS for ell in s.ells for ps in POSES]


def dense_case(pkg, po, name, n, m, ell, pose_):
    """One dense case: iteration_ref_cases.clouds(n, m) of the set's mode at a pose of iteration_ref_cases.poses(ell), the
    oracle's members and the float64 reference, with the borderline count asserted."""
    s = BY_NAME[name]
    p = s.params(po)
    _, R, T = pose_
    xf, ff, xm, fm = ic.clouds(pkg, s.mode, n, m)
    y = po.transform(R, T, xm)
    rp, cols, val = po.se_kernel(p, ell, xf, ff, y, fm, search=search_of(po, s))
    rows = np.repeat(np.arange(n), np.diff(rp))
    a, d2, d2c, margin = ref.weights(p, ell, xf, ff, y, fm, c_sp=ic.c_sp_of(p))
    sure_in, border, sure_out = ref.classify(margin)
    assert int(border.sum()) <= DENSE_BORDER_MAX * n * m, (name, n, m, ell, pose_[0], int(border.sum()))
    return dict(set=s, p=p, ell=ell, R=R, T=T, xf=xf, ff=ff, xm=xm, fm=fm, y=y, csr=(rp, cols, val), rows=rows, cols=cols,
                val=val, a=a, d2=d2, d2c=d2c, margin=margin, sure_in=sure_in, border=border, sure_out=sure_out)


def dense_ell(s):
    """The length scale a set's dense pairs run at: its first."""
    return s.ells[0]
