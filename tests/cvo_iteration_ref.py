"""Float64 restatement of one CVO / Adaptive-CVO iteration's O(N.M) arithmetic, written from the reference's equations on
dense N x M numpy arrays: the pair weight and its three cuts, the twist sums of compute_flow, acvo's length-scale
derivative, function_inner_product and every term of compute_step_size's B, C, D, E.

Reference lines followed (paths under cpp/rkhs_registration/ and matlab/@rkhs_se3_registration/):
    src/cvo.cpp:99-161            se_kernel           src/cvo.cpp:164-210           compute_flow
    src/cvo.cpp:213-308           compute_step_size   src/adaptive_cvo.cpp:92-151   se_kernel (c_sp_thres)
    src/adaptive_cvo.cpp:154-272  compute_flow + dl   src/adaptive_cvo.cpp:385-439  function_inner_product
    rkhs_se3_registration.m:40-73,125-127             the MATLAB object's weight

A plain module shared by tests/test_iteration_ref_cpu.py (the oracle against this) and tests/test_gpu_iteration_ref.py
(the kernels against this).  It knows nothing of the oracle or the library: numpy float64 only.  Inputs are the float32
clouds, features and parameters exactly as given, converted to float64; nothing here imitates float32 rounding.  Next to
every sum it returns the sum of the absolute values of the products the sum is made of ("scale"): the magnitude that the
float32 rounding of the per-pair terms on the other side is relative to.
"""
import numpy as np

BAND = 1e-5   # |margin| below this: the pair is borderline (see weights())


def _f(v):
    """A float32 parameter (or array) as float64, value unchanged."""
    return np.asarray(v, np.float32).astype(np.float64)


def _par(p, name):
    return float(np.float32(getattr(p, name)))


def cuts(p, ell, c_sp, two_divisions=False):
    """(tau, tau_c): the squared-distance thresholds the sparsification threshold is converted to,
        tau = -2 l^2 ln(sp / s2),   tau_c = -2 c_l^2 ln(c_sp / c_sigma / c_sigma)
    (cvo.cpp:102-103, adaptive_cvo.cpp:100-101; c_sp is sp_thres in cvo and c_sp_thres in acvo).  two_divisions: the
    spatial quotient written sp / sigma / sigma as adaptive_cvo.cpp:391 has it."""
    ell, c_sp = float(np.float32(ell)), float(np.float32(c_sp))
    sigma, sp, c_ell, c_sigma = _par(p, "sigma"), _par(p, "sp_thres"), _par(p, "c_ell"), _par(p, "c_sigma")
    q = sp / sigma / sigma if two_divisions else sp / (sigma * sigma)
    return -2.0 * ell * ell * np.log(q), -2.0 * c_ell * c_ell * np.log(c_sp / c_sigma / c_sigma)


def sq_dists(xa, xb):
    """Dense |a_i - b_j|^2 from the differences (no expansion of the square: nothing cancels)."""
    e = _f(xa)[:, None, :] - _f(xb)[None, :, :]
    return np.einsum("ijk,ijk->ij", e, e)


def weights(p, ell, x, fx, y, fy, c_sp, two_divisions=False):
    """Dense (a, d2, d2c, margin) of the cloud x (N) against y (M), all N x M float64.

    The C++ weight (cvo.cpp:143-153, adaptive_cvo.cpp:134-144): with d2 = |x_i - y_j|^2 and d2c = |f_i - g_j|^2 over the
    five features,
        k = s2 exp(-d2 / 2 l^2),  ck = c_sigma^2 exp(-d2c / 2 c_l^2),  a = ck k,
    kept iff d2 < tau and d2c < tau_c and a > sp_thres.
    The MATLAB weight (p.color_scale > 0; rkhs_se3_registration.m:52,72,126-127): K = s2 exp(-d2 / 2 l^2) is set to zero
    where K < sp_threshold, and a = color_scale <c_i, c_j> K with c the first three features; kept iff K >= sp (d2c is
    returned but cuts nothing) and a != 0: A = sparse(CI .* K) stores no zero (:127), so a black point has no member.

    a is the weight whether the pair is kept or not.  margin is the signed relative distance to the nearest cut, negative
    inside: the largest of d2 / tau - 1, d2c / tau_c - 1 and sp / a - 1 (MATLAB: sp / K - 1 alone, and +inf where a = 0).
    A pair is kept iff margin < 0 (MATLAB: <= 0; see kept()); it is surely in when margin < -BAND, surely out when margin > BAND, borderline otherwise.
    BAND is 1e-5 because the cut values on the float32 side are float32 (relative 6e-8) and d2, d2c carry a few float32
    roundings there: two orders of magnitude of room."""
    ell = float(np.float32(ell))
    s2, cs2, sp = _par(p, "sigma") ** 2, _par(p, "c_sigma") ** 2, _par(p, "sp_thres")
    c_ell, cscale = _par(p, "c_ell"), _par(p, "color_scale")
    tau, tau_c = cuts(p, ell, c_sp, two_divisions)
    d2 = sq_dists(x, y)
    e = _f(fx)[:, None, :] - _f(fy)[None, :, :]
    d2c = np.einsum("ijk,ijk->ij", e, e)
    k = s2 * np.exp(-d2 / (2.0 * ell * ell))
    with np.errstate(divide="ignore", over="ignore"):
        if cscale > 0.0:
            a = cscale * (_f(fx)[:, :3] @ _f(fy)[:, :3].T) * k
            margin = np.where(a != 0.0, sp / k - 1.0, np.inf)
        else:
            a = cs2 * np.exp(-d2c / (2.0 * c_ell * c_ell)) * k
            # (a threshold at or above sigma^2 or c_sigma^2 makes tau or tau_c zero or negative: d2 < tau holds for no pair)
            m1 = d2 / tau - 1.0 if tau > 0.0 else np.full_like(d2, np.inf)
            m2 = d2c / tau_c - 1.0 if tau_c > 0.0 else np.full_like(d2c, np.inf)
            margin = np.maximum(np.maximum(m1, m2), sp / a - 1.0)
    return a, d2, d2c, margin


def kept(p, margin):
    """The reference's own member set as a boolean N x M array: margin < 0, for the MATLAB weight margin <= 0."""
    return margin <= 0.0 if _par(p, "color_scale") > 0.0 else margin < 0.0


def classify(margin):
    """(surely in, borderline, surely out) as boolean arrays."""
    return margin < -BAND, np.abs(margin) <= BAND, margin > BAND


def _cross_scale(ax, ay):
    return np.stack([ax[:, 1] * ay[:, 2] + ax[:, 2] * ay[:, 1], ax[:, 2] * ay[:, 0] + ax[:, 0] * ay[:, 2],
                     ax[:, 0] * ay[:, 1] + ax[:, 1] * ay[:, 0]], 1)


def flow(p, ell, x, y, rows, cols, a):
    """compute_flow's sums over the members (rows[q], cols[q]) with weights a[q] (cvo.cpp:188-203,
    adaptive_cvo.cpp:197-228):
        omega_d = sum (1/c) a x_i cross y_j,   v_d = sum (1/d) a (y_j - x_i),
        sum_a = sum a,   sum_a_d2 = sum (1/l^3) a |y_j - x_i|^2   (the Axy part of acvo's dl, without its factor -2).
    s_omega, s_v, s_a, s_a_d2 are the scales: for the cross product sum (a/c)(|x_k y_l| + |x_l y_k|); for the difference
    |y - x| itself (a float32 subtraction rounds relative to its result)."""
    ell = float(np.float32(ell))
    c, d = _par(p, "c"), _par(p, "d")
    X, Y, a = _f(x)[rows], _f(y)[cols], np.asarray(a, np.float64)
    df = Y - X
    d2 = np.einsum("nk,nk->n", df, df)
    l3 = ell * ell * ell
    return dict(omega_d=(1.0 / c) * (a[:, None] * np.cross(X, Y)).sum(0), v_d=(1.0 / d) * (a[:, None] * df).sum(0),
                sum_a=float(a.sum()), sum_a_d2=float((a * d2).sum() / l3),
                s_omega=(1.0 / c) * (np.abs(a)[:, None] * _cross_scale(np.abs(X), np.abs(Y))).sum(0),
                s_v=(1.0 / d) * (np.abs(a)[:, None] * np.abs(df)).sum(0),
                s_a=float(np.abs(a).sum()), s_a_d2=float((np.abs(a) * d2).sum() / l3))


def dl(ell, x, y, A, Axx, Ayy):
    """acvo's length-scale derivative (adaptive_cvo.cpp:171-271).  A, Axx, Ayy: (rows, cols, weights) of the members of
    x against y, x against x and y against y; N = len(x), M = len(y).

        dl = [ S_yy - 2 S_xy + S_xx ] / (nnz(Axx) + nnz(Ayy) - 2 nnz(A)),   S = sum (1/l^3) a |b_j - a_i|^2.

    The row rule: rows i < min(N, M) of Ayy go through the main loop (:213-223), rows N <= i < M through the tail loop
    (:243-265).  The main loop fills diff_yy but never sum_diff_yy_2, which stays the zero it was created as (:190), so
    its product Ayyi * sum_diff_yy_2 (:222) is zero; only the tail loop computes the squared norms (:256).  Followed here as
    the text has it: S_yy runs over the Ayy rows i >= N alone, and is zero when M <= N.  (The oracle and the kernels take
    the same reading: cvo_oracle.c self_rows with first_counted = N.)  The counts in the denominator are of all members.

    Returns dl, the three contributions s_yy, s_xy, s_xx (s_xy without the factor -2), what the main-loop rows of Ayy
    would have added had :219 filled the norms (s_yy_main), den, and scale = s_yy + 2 s_xy + s_xx (every term is
    non-negative, so the contributions are their own scales)."""
    ell = float(np.float32(ell))
    l3 = ell * ell * ell
    N = len(x)

    def S(pa, pb, members, keep=None):
        r, c, a = members
        e = _f(pb)[c] - _f(pa)[r]
        t = np.asarray(a, np.float64) * np.einsum("nk,nk->n", e, e) / l3
        return float(t.sum() if keep is None else t[keep(np.asarray(r))].sum())

    s_xy, s_xx = S(x, y, A), S(x, x, Axx)
    s_yy = S(y, y, Ayy, lambda r: r >= N)            # the tail loop
    s_yy_main = S(y, y, Ayy, lambda r: r < N)        # the main loop's rows: zero in the reference
    den = len(Axx[0]) + len(Ayy[0]) - 2 * len(A[0])
    num = s_yy - 2.0 * s_xy + s_xx
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(dl=float(np.float64(num) / np.float64(den)), s_yy=s_yy, s_xy=s_xy, s_xx=s_xx, s_yy_main=s_yy_main,
                    den=den, scale=s_yy + 2.0 * s_xy + s_xx)


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


STEP_TERMS = ("B_beta", "C_gamma", "C_beta2", "D_delta", "D_beta_gamma", "D_beta3", "E_epsil", "E_beta_delta",
              "E_beta2_gamma", "E_gamma2", "E_beta4")
COEFF_OF = dict(B_beta=0, C_gamma=1, C_beta2=1, D_delta=2, D_beta_gamma=2, D_beta3=2, E_epsil=3, E_beta_delta=3,
                E_beta2_gamma=3, E_gamma2=3, E_beta4=3)
# the inner summands of gamma, delta and epsil (cvo.cpp:264-271), each times a: parts of C_gamma, D_delta and E_epsil
SUB_TERMS = ("C_gamma.xiz2", "C_gamma.xi2z_df", "D_delta.xiz_xi2z", "D_delta.xi3z_df", "E_epsil.xi2z2", "E_epsil.xiz_xi3z",
             "E_epsil.xi4z_df")


def _dot(p, q):
    return np.einsum("nk,nk->n", p, q)


def _step_members(ell, W, v, Y, df, sign=-1.0):
    """beta, gamma, delta, epsil per member and the inner summands of the last three, from omega_hat = W, v, the moving
    points Y and df = x - y, by cvo.cpp:226-238,260-271 as written:
        xiz = omega cross y + v,  xi2z = W W y + W v,  xi3z = W W W y + W W v,  xi4z = W^4 y + W^3 v
    -- without the factorials 1/2, 1/6, 1/24 of the exponential's series: fidelity to the reference, not to the series --
        beta  = -(1/l^2) xiz.df                               gamma = -(1/2l^2) (|xiz|^2 + 2 xi2z.df)
        delta =  (1/l^2) (-xiz.xi2z - xi3z.df)                epsil = -(1/2l^2) (|xi2z|^2 + 2 xiz.xi3z + 2 xi4z.df).
    sign = +1 gives the absolute versions: every minus sign becomes a plus (the inputs are then absolute values too)."""
    tc = 1.0 / (2.0 * ell * ell)
    W2 = W @ W
    W3 = W2 @ W
    W4 = W3 @ W
    xiz = Y @ W.T + v
    xi2z = Y @ W2.T + W @ v
    xi3z = Y @ W3.T + W2 @ v
    xi4z = Y @ W4.T + W3 @ v
    beta = sign * 2.0 * tc * _dot(xiz, df)
    sub = {"C_gamma.xiz2": sign * tc * _dot(xiz, xiz), "C_gamma.xi2z_df": sign * tc * 2.0 * _dot(xi2z, df),
           "D_delta.xiz_xi2z": sign * 2.0 * tc * _dot(xiz, xi2z), "D_delta.xi3z_df": sign * 2.0 * tc * _dot(xi3z, df),
           "E_epsil.xi2z2": sign * tc * _dot(xi2z, xi2z), "E_epsil.xiz_xi3z": sign * tc * 2.0 * _dot(xiz, xi3z),
           "E_epsil.xi4z_df": sign * tc * 2.0 * _dot(xi4z, df)}
    gamma = sub["C_gamma.xiz2"] + sub["C_gamma.xi2z_df"]
    delta = sub["D_delta.xiz_xi2z"] + sub["D_delta.xi3z_df"]
    epsil = sub["E_epsil.xi2z2"] + sub["E_epsil.xiz_xi3z"] + sub["E_epsil.xi4z_df"]
    return beta, gamma, delta, epsil, sub


def _step_products(a, beta, gamma, delta, epsil):
    """The products of cvo.cpp:275-279 per member, in STEP_TERMS order."""
    return dict(B_beta=a * beta, C_gamma=a * gamma, C_beta2=a * beta * beta / 2.0,
                D_delta=a * delta, D_beta_gamma=a * beta * gamma, D_beta3=a * beta ** 3 / 6.0,
                E_epsil=a * epsil, E_beta_delta=a * beta * delta, E_beta2_gamma=a * beta * beta * gamma / 2.0,
                E_gamma2=a * gamma * gamma / 2.0, E_beta4=a * beta ** 4 / 24.0)


def step_terms(ell, omega, v, x, y, rows, cols, a):
    """compute_step_size's coefficient sums over the members (cvo.cpp:226-280).  Returns
        beta, gamma, delta, epsil   per member (_step_members),
        terms   the products of cvo.cpp:275-279 summed over the members, each kept apart (STEP_TERMS) --
                B: a beta | C: a gamma, a beta^2/2 | D: a delta, a beta gamma, a beta^3/6 |
                E: a epsil, a beta delta, a beta^2 gamma/2, a gamma^2/2, a beta^4/24: 1 + 2 + 3 + 5 = 11 sums --
                and, under SUB_TERMS, the seven inner summands of gamma, delta and epsil times a,
        bcde    B, C, D, E,
        scales  per term and sub-term, the same sums with every elementary product replaced by its absolute value
                (|omega_hat|, |v|, |y|, |x - y| throughout, every minus a plus): what a float32 evaluation's roundings
                are relative to,
        coeff_scales  those of a coefficient's terms added up: (4,)."""
    ell = float(np.float32(ell))
    w, v = _f(omega), _f(v)
    X, Y, a = _f(x)[rows], _f(y)[cols], np.asarray(a, np.float64)
    df = X - Y
    beta, gamma, delta, epsil, sub = _step_members(ell, _hat(w), v, Y, df)
    terms = {k: float(t.sum()) for k, t in _step_products(a, beta, gamma, delta, epsil).items()}
    terms.update({k: float((a * t).sum()) for k, t in sub.items()})
    bcde = np.zeros(4)
    for k in STEP_TERMS:
        bcde[COEFF_OF[k]] += terms[k]
    sb, sg, sd, se, ssub = _step_members(ell, np.abs(_hat(w)), np.abs(v), np.abs(Y), np.abs(df), sign=1.0)
    aa = np.abs(a)
    scales = {k: float(t.sum()) for k, t in _step_products(aa, sb, sg, sd, se).items()}
    scales.update({k: float((aa * t).sum()) for k, t in ssub.items()})
    coeff_scales = np.zeros(4)
    for k in STEP_TERMS:
        coeff_scales[COEFF_OF[k]] += scales[k]
    return dict(beta=beta, gamma=gamma, delta=delta, epsil=epsil, terms=terms, bcde=bcde, scales=scales,
                coeff_scales=coeff_scales)


def function_inner_product(p, ell, xa, fa, xb, fb):
    """acvo::function_inner_product (adaptive_cvo.cpp:385-439): the mean of the kept weights of cloud a against cloud b on
    the positions as given.  Its own threshold lines: the colour cut is formed from sp_thres (:392), not from c_sp_thres as
    acvo's se_kernel forms it (:101), and the spatial quotient is sp_thres / sigma / sigma (:391).  Returns (value, sum of
    kept weights, count, margin); 0 / 0 is NaN as in the reference."""
    a, _, _, margin = weights(p, ell, xa, fa, xb, fb, _par(p, "sp_thres"), two_divisions=True)
    keep = margin < 0.0
    s, n = float(a[keep].sum()), int(keep.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(s) / np.float64(n)), s, n, margin
