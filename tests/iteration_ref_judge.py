"""The judge of one flow / step pass: the float64 reference of a cloud pair at one length scale over its OWN members, the
borderline pairs, and the checks that hold thirteen flow outputs and four step coefficients to it.  Moved here from
tests/test_gpu_iteration_ref.py (whose assertions are these, unchanged) so that the row-sharded tests
(tests/test_gpu_shard_ref.py, tests/test_shard_ref_cpu.py) and tools/gpu_ranks_threads.py apply the same judge.  A plain
module; no test lives here.

A row range: Ref.shard(lo, hi) is the same reference over the members whose row lies in [lo, hi) -- what a context with
cvo_hip_set_shard(lo, hi, ...) sums.  The Ayy sum of acvo's dl counts a member only if the CALLER's index of its row is
>= first_counted (adaptive_cvo.cpp:243-265: rows N <= i < M of the cloud as the caller handed it over); `row_ids` gives that
index for every row of a cloud that is held in another order (the device's Morton order: Context.device_cloud), and is
the row itself where none is given.
"""
import numpy as np
import pytest

import cvo_iteration_ref as ref
import iteration_ref_cases as ic


class Ref:
    """The reference of one cloud pair at one length scale: its own members, the borderline pairs, the float64 weights."""

    def __init__(self, p, ell, xa, fa, xb, fb, row_ids=None):
        self.p, self.ell, self.xa, self.xb = p, ell, xa, xb
        self.a, _, _, margin = ref.weights(p, ell, xa, fa, xb, fb, c_sp=ic.c_sp_of(p))
        self.rows, self.cols = ic.dense_members(p, margin)
        sure_in, border, _ = ref.classify(margin)
        self.sure_rows = sure_in.sum(axis=1)
        self.sure_in, self.brows, self.bcols = int(sure_in.sum()), *np.nonzero(border)
        self.am = self.a[self.rows, self.cols]
        self.row_ids = np.arange(len(xa)) if row_ids is None else np.asarray(row_ids)
        self.lo, self.hi = 0, len(xa)

    def shard(self, lo, hi):
        """The same reference over the members (and the borderline pairs) of the rows lo <= row < hi."""
        import copy
        s = copy.copy(self)
        lo, hi = max(0, min(lo, len(self.xa))), max(0, min(hi, len(self.xa)))
        keep, bkeep = (self.rows >= lo) & (self.rows < hi), (self.brows >= lo) & (self.brows < hi)
        s.rows, s.cols, s.am = self.rows[keep], self.cols[keep], self.am[keep]
        s.brows, s.bcols = self.brows[bkeep], self.bcols[bkeep]
        s.sure_in = int(self.sure_rows[lo:hi].sum()) if hi > lo else 0
        s.lo, s.hi = lo, hi
        return s

    def count_ok(self, nnz):
        return self.sure_in <= int(nnz) <= self.sure_in + len(self.brows)

    def flow(self):
        fl = ref.flow(self.p, self.ell, self.xa, self.xb, self.rows, self.cols, self.am)
        tol = ic.flow_tol(self.p, fl)
        if len(self.brows):
            b = ref.flow(self.p, self.ell, self.xa, self.xb, self.brows, self.bcols, self.a[self.brows, self.bcols])
            for k, s in (("omega_d", "s_omega"), ("v_d", "s_v"), ("sum_a", "s_a"), ("sum_a_d2", "s_a_d2")):
                tol[k] = tol[k] + b[s]
        return fl, tol

    def step(self, omega, v):
        st = ref.step_terms(self.ell, omega, v, self.xa, self.xb, self.rows, self.cols, self.am)
        tol = ic.step_tol(self.p, st)
        if len(self.brows):
            tol = tol + ref.step_terms(self.ell, omega, v, self.xa, self.xb, self.brows, self.bcols,
                                       self.a[self.brows, self.bcols])["coeff_scales"]
        return st, tol

    def self_flow(self, first_row=0):
        """cvo_iteration_ref.flow over the members whose row's caller index is >= first_row."""
        keep = self.row_ids[self.rows] >= first_row
        return ref.flow(self.p, self.ell, self.xa, self.xb, self.rows[keep], self.cols[keep], self.am[keep])

    def self_sum(self, first_row=0):
        """(sum (1/l^3) a d2 over the members in rows >= first_row, its tolerance): the Axx / Ayy sums of dl."""
        fl = self.self_flow(first_row)
        tol = ic.flow_tol(self.p, fl)["sum_a_d2"]
        if len(self.brows):
            tol += ref.flow(self.p, self.ell, self.xa, self.xb, self.brows, self.bcols, self.a[self.brows, self.bcols])["s_a_d2"]
        return fl["sum_a_d2"], tol


def _see(worst, key, err, tol):
    if worst is not None:
        worst.see(key, err, tol)


def check_flow(out, R_, worst=None):
    fl, tol = R_.flow()
    _see(worst, "omega_d", np.abs(out[0:3] - fl["omega_d"]), tol["omega_d"])
    _see(worst, "v_d", np.abs(out[3:6] - fl["v_d"]), tol["v_d"])
    _see(worst, "sum_a", abs(out[6] - fl["sum_a"]), tol["sum_a"])
    _see(worst, "sum_a_d2", abs(out[7] - fl["sum_a_d2"]), tol["sum_a_d2"])
    assert R_.count_ok(out[8]), (out[8], R_.sure_in, len(R_.brows), R_.lo, R_.hi)
    assert np.all(np.abs(out[0:3] - fl["omega_d"]) <= tol["omega_d"]), (out[0:3], fl["omega_d"], tol["omega_d"])
    assert np.all(np.abs(out[3:6] - fl["v_d"]) <= tol["v_d"]), (out[3:6], fl["v_d"], tol["v_d"])
    assert abs(out[6] - fl["sum_a"]) <= tol["sum_a"] and abs(out[7] - fl["sum_a_d2"]) <= tol["sum_a_d2"]
    return fl


def check_step(pkg, c, R_, omega, v, ell, worst=None):
    bcde = c.step_coeffs(omega, v, ell)
    st, tol = R_.step(omega, v)
    _see(worst, "bcde", np.abs(bcde - st["bcde"]), tol)
    assert np.all(np.abs(bcde - st["bcde"]) <= tol), (bcde, st["bcde"], tol, R_.lo, R_.hi)
    want = ic.roots_step(bcde)
    if want is not None:
        assert pkg.capi.pick_step(bcde) == pytest.approx(want, rel=1e-5), bcde
    return bcde, st


def check_self(out, k, S_, first_row=0, worst=None):
    """out[k], out[k + 1] of cvo_hip_flow (k = 9: Axx, k = 11: Ayy) against the self reference S_: the sum over the counted rows,
    the count over all of them."""
    want, tol = S_.self_sum(first_row)
    _see(worst, "self_sum", abs(out[k] - want), tol)
    assert S_.count_ok(out[k + 1]), (k, out[k + 1], S_.sure_in, S_.lo, S_.hi)
    assert abs(out[k] - want) <= tol, (k, out[k], want, tol, S_.lo, S_.hi)
    return want
