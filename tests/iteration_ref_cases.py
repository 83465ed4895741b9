"""What tests/test_iteration_ref_cpu.py and tests/test_gpu_iteration_ref.py share: the cases, the poses, and the tolerances
that hold a float32 evaluation (the oracle's, the kernels') to the float64 reference of tests/cvo_iteration_ref.py.  A plain
module; no test lives here.

How the tolerances are derived.  u = 2^-24 is the unit roundoff of float32.  A quantity q evaluated in float32 is followed
through its chain with a count K(q) of roundings and a majorant S(q) -- q with every elementary product replaced by its
absolute value -- such that |fl(q) - q| <= K(q) u S(q) to first order in u:
    inputs (coordinates, features, the twist) are exact: K = 0;
    fl(q r):   K = K(q) + K(r) + 1,        S = S(q) S(r);
    fl(q + r): K = max(K(q), K(r)) + 1,    S = S(q) + S(r);
    a float32 difference of two inputs rounds relative to its own result: K = 1, S = |q - r|;
    a conversion to float64 and everything in float64 after it: nothing (2^-53 against 2^-24).
A sum over the members of such terms, accumulated in float64, is then within K u sum S of the float64 sum.  No figure
below comes from an observed error.

The weight (cvo_oracle.c pair_weight; the kernels' cvo_pair.h is held to it bit for bit elsewhere):
    s2 = fl(sigma sigma) 1, cs2 likewise 1, k = fl(s2 exp(.)) 1, ck 1, a = fl(ck k) 1: 5 roundings;
    d2 = three squared float32 differences (2 each) through a square and two fused multiply-adds (<= 3): 5 u relative, all
    terms being non-negative; d2c = five of them through a square and four fused multiply-adds: 7 u relative; the
    exponentials turn these into 5 u E1 and 7 u E2 relative, E1 = d2 / 2 l^2, E2 = d2c / 2 c_l^2 the exponents' magnitudes;
    -> |val - a| <= u (5 + 5 E1 + 7 E2) a per pair.
    For a kept pair a > sp, so E1 + E2 < ln(s2 cs2 / sp) and, for use inside the sums,
    KW = 5 + 7 ln(s2 cs2 / sp)        (cvo 6.6, acvo 6.3).
    (The two separate cuts give ln(s2 / sp) for E1 and ln(cs2 / c_sp) for E2; the third cut is the tighter statement of E2.)
The MATLAB weight: the colour inner product of three non-negative products (1 each) through two additions: 3; times
    color_scale 1; s2 1; K 1; the product 1: 7 roundings, and 5 u E1 with E1 <= ln(s2 / sp) (1 + 1e-5):
    KW = 7 + 5 ln(s2 / sp) + 1e-4     (18.5 with the MATLAB object's constants).

compute_flow (cvo_oracle.c flow_rows), per pair and component:
    omega: fl(fl(1/c) val) fl(fl(x_k y_l) - fl(x_l y_k)): 1/c 1, times val 1, two products 1, their difference 1, the last
           product 1                                                                  K = KW + 5, S = (a/c)(|x_k y_l| + |x_l y_k|)
    v:     1/d 1, times val 1, fl(y - x) 1, the product 1                             K = KW + 4, S = (a/d)|y_k - x_k|
    sum_a: the weights added in float64                                               K = KW,     S = a
    sum_a_d2 (and the Axx, Ayy sums of dl): l^3 2, its reciprocal 1, times val 1, d2 5, the product 1
                                                                                      K = KW + 10, S = a d2 / l^3
compute_step_size (cvo_oracle.c taylor_point, step_rows), W = omega_hat, majorants with |W|, |v|, |y|, |x - y|:
    df = fl(x - y) 1;  omega cross y 2, + v: xiz 3;
    W W: products 1, two additions: 3; (W W) W: 3 + 1 + 2 = 6; W^4: 9;  W v 3, W W v 6, W^3 v 9;
    xi2z = fl(W2 y + W v): 3 + 1 + 2 = 6, max(6, 3) + 1 = 7;  xi3z: 6 + 3 = 9, + 1 = 10;  xi4z: 9 + 3 = 12, + 1 = 13;
    temp_coef = 1 / (2 l^2) stored as float: 1 (and its multiples by 2 exactly);
    beta  = sum_k fl(fl(cb xiz_k) df_k): 1 + 3 + 1 = 5, + 1 + 1 = 7, two additions:                            K_beta  = 9
    gamma = cg (|xiz|^2 [3 + 3 + 1 + 2 = 9] + 2 xi2z.df [7 + 1 + 1 + 2 = 11]): 12, times cg: + 1 + 1           K_gamma = 14
    delta = cd (-xiz.xi2z [3 + 7 + 1 + 2 = 13] - xi3z.df [10 + 1 + 1 + 2 = 14]): 15, + 2                       K_delta = 17
    epsil = cg (|xi2z|^2 [7 + 7 + 1 + 2 = 17] + 2 xiz.xi3z [3 + 10 + 1 + 2 = 16]: 18; + 2 xi4z.df [13 + 4 = 17]): 19, + 2
                                                                                                               K_epsil = 21
    and the products of cvo.cpp:275-279 with the C promotions the oracle spells out (float products, then float64):
    B: fl(a beta)                         KW + 9 + 1                 = KW + 10
    C: a gamma                            KW + 14;    a fl(beta beta) / 2        KW + 18 + 1         = KW + 19
    D: a fl(delta + fl(beta gamma)):      delta KW + 17 + 1 = KW + 18;   beta gamma KW + (9 + 14 + 1) + 1 = KW + 25;
       a fl(fl(beta beta) beta) / 6       KW + 27 + 2                = KW + 29
    E: a fl(epsil + fl(beta delta)):      epsil KW + 22;   beta delta KW + (9 + 17 + 1) + 1 = KW + 28;
       beta beta gamma / 2 in float64     KW + 18 + 14 = KW + 32;   gamma^2 / 2   KW + 28;   beta^4 / 24   KW + 36
    Each coefficient's tolerance is u sum over its terms of K_term S_term.
"""
import numpy as np

import cvo_iteration_ref as ref

U = 2.0 ** -24

SIZES = [(257, 63), (300, 260), (260, 300), (64, 1), (1, 300)]
ELLS = [0.15, 0.1, 0.06, 0.03]
MODES = ["cvo", "acvo", "matlab"]
TWIST_SCALES = [0.02, 0.3, 1.0]
# Two more acvo parameter sets.  At the shipped constants two of the three cuts never decide a pair: a > sp with ck <= 1
# implies k > sp, which is d2 < tau; and it implies ck > sp / s2 = 0.83, which is tighter than the colour cut's
# ck > c_sp_thres = 0.0083.  c_sp_thres = 0.98 lets the colour cut remove pairs of its own; c_sigma = 1.25 (ck up to 1.56)
# lets the radius do so.  Each with the length scales it is run at, on (300, 260) and (260, 300).  (At ell = 0.15 and the small
# motion one pair of (300, 260) lies within 1e-5 of the radius; the shipped constants' a > sp removes it long before, c_sigma =
# 1.25 would leave it borderline: hence other length scales there.)
ACVO_VARIANTS = [(dict(c_sp_thres=0.98), (0.15, 0.1)), (dict(c_sigma=1.25), (0.12, 0.07))]

K_FLOW = dict(omega=5, v=4, sum_a=0, sum_a_d2=10)
K_STEP = dict(B_beta=10, C_gamma=14, C_beta2=19, D_delta=18, D_beta_gamma=25, D_beta3=29, E_epsil=22, E_beta_delta=28,
              E_beta2_gamma=32, E_gamma2=28, E_beta4=36)


def small_motion():
    """tests/test_gpu_parity.py _small_motion."""
    R = np.eye(3, dtype=np.float32)
    th = 0.01
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    return R, np.array([0.002, -0.001, 0.003], np.float32)


def poses(ell):
    """identity, the small motion, and the small rotation with a translation of about one ell (|x - y| ~ ell for the
    members that remain: beta is not small)."""
    R, T = small_motion()
    return [("identity", np.eye(3, dtype=np.float32), np.zeros(3, np.float32)), ("small", R, T),
            ("one_ell", R, (np.float32(ell) * np.array([0.6, -0.5, 0.62], np.float32)).astype(np.float32))]


def mode_id(api, mode):
    return {"cvo": api.MODE_CVO, "acvo": api.MODE_ACVO, "matlab": api.MODE_MATLAB}[mode]


def clouds(pkg, mode, n, m):
    """data.synthetic_pair(n, m, seed=11): the acvo feature scale in acvo mode; for the MATLAB weight the raw B, G, R of the
    cvo scale are the colours (non-negative, as the derivation of KW requires)."""
    xf, ff, xm, fm = pkg.data.synthetic_pair(n, m, seed=11, acvo=(mode == "acvo"))
    assert ff[:, :3].min() >= 0 and fm[:, :3].min() >= 0
    return xf, ff, xm, fm


def c_sp_of(p):
    """The colour cut's threshold in se_kernel: c_sp_thres in acvo (adaptive_cvo.cpp:101), sp_thres in cvo (cvo.cpp:103)."""
    return p.c_sp_thres if p.mode == 1 else p.sp_thres


def kw(p):
    s2, cs2, sp = float(np.float32(p.sigma)) ** 2, float(np.float32(p.c_sigma)) ** 2, float(np.float32(p.sp_thres))
    if p.color_scale > 0:
        return 7.0 + 5.0 * np.log(s2 / sp) + 1e-4
    return 5.0 + 7.0 * np.log(s2 * cs2 / sp)


def weight_bound(p, ell, a, d2, d2c):
    """Per pair, the absolute bound on |float32 weight - a| (module docstring)."""
    ell, c_ell = float(np.float32(ell)), float(np.float32(p.c_ell))
    if p.color_scale > 0:
        return U * (7.0 + 5.0 * d2 / (2.0 * ell * ell)) * np.abs(a)
    return U * (5.0 + 5.0 * d2 / (2.0 * ell * ell) + 7.0 * d2c / (2.0 * c_ell * c_ell)) * np.abs(a)


def flow_tol(p, fl):
    """Tolerances of omega_d (3,), v_d (3,), sum_a, sum_a_d2 from cvo_iteration_ref.flow's scales."""
    k = kw(p)
    return dict(omega_d=(k + K_FLOW["omega"]) * U * fl["s_omega"], v_d=(k + K_FLOW["v"]) * U * fl["s_v"],
                sum_a=(k + K_FLOW["sum_a"]) * U * fl["s_a"], sum_a_d2=(k + K_FLOW["sum_a_d2"]) * U * fl["s_a_d2"])


def step_tol(p, st):
    """(4,) tolerances of B, C, D, E from cvo_iteration_ref.step_terms' scales."""
    k = kw(p)
    tol = np.zeros(4)
    for t in ref.STEP_TERMS:
        tol[ref.COEFF_OF[t]] += (k + K_STEP[t]) * U * st["scales"][t]
    return tol


def dl_tol(p, d):
    """dl's tolerance: the three sums' (KW + 10) u scale over the denominator (exact integers)."""
    return (kw(p) + K_FLOW["sum_a_d2"]) * U * d["scale"] / abs(d["den"]) if d["den"] != 0 else np.inf


def twists(seed):
    """omega, v ~ N(0, s) for s in TWIST_SCALES, float32."""
    rng = np.random.default_rng(seed)
    return [(s, rng.normal(0, s, 3).astype(np.float32), rng.normal(0, s, 3).astype(np.float32)) for s in TWIST_SCALES]


def dense_members(p, margin):
    """(rows, cols) of the reference's own member set, in CSR order."""
    rows, cols = np.nonzero(ref.kept(p, margin))
    return rows, cols


def cubic_roots(bcde):
    """(positive real roots, nearly_double) of the cubic of cvo.cpp:291-296 as numpy.roots finds them on the monic form with
    float32-rounded ratios, or None for a degenerate cubic (E == 0 as a float, or a coefficient that is not finite)."""
    c = np.array([4.0 * np.float32(bcde[3]), 3.0 * np.float32(bcde[2]), 2.0 * np.float32(bcde[1]), np.float32(bcde[0])],
                 np.float32).astype(np.float64)
    if c[0] == 0.0 or not np.all(np.isfinite(c)):
        return None
    mon = np.array([1.0, np.float32(c[1] / c[0]), np.float32(c[2] / c[0]), np.float32(c[3] / c[0])], np.float64)
    r = np.roots(mon)
    real = r[np.abs(r.imag) < 1e-9 * np.maximum(1.0, np.abs(r.real))].real
    cplx = r[np.abs(r.imag) >= 1e-9 * np.maximum(1.0, np.abs(r.real))]
    near = bool(len(cplx) and np.min(np.abs(cplx.imag) / np.maximum(1.0, np.abs(cplx.real))) < 1e-5)
    return real[real > 0], near


def roots_step(bcde, min_step=np.float32(0.2)):
    """The step tests/test_host_math.py test_pick_step_matches_numpy_roots expects for float64 coefficients, or None where
    that test skips (nearly a double root) -- and for a degenerate cubic, which that test's random draws never meet."""
    found = cubic_roots(bcde)
    if found is None or found[1]:
        return None
    pos = found[0]
    want = np.float32(pos.min()) if len(pos) else np.float32(min_step)
    return float(np.float32(0.8) if want > 0.8 else want)
