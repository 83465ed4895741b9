"""What tests/test_shard_ref_cpu.py, tests/test_gpu_shard_ref.py and tools/gpu_ranks_threads.py share: ONE definition of the
row cuts, the judges that hold a row shard (and a registration of several of them) to the float64 references of
tests/cvo_iteration_ref.py and tests/cvo_loop_ref.py, the oracle standing in for the library behind the same calls, and
the mutants of the driver.  A plain module; no test lives here.

The cuts.  A cut list c_0 = 0 <= c_1 <= ... <= c_W over a cloud of n rows gives rank r the rows [c_r, c_r+1); the last
rank's end may lie beyond n (cvo_plan.cpp shard_ranges clamps it) and a rank whose range is empty after the clamps takes
part in every exchange with zeros.  Rows are DEVICE rows: the clouds are in Morton order after the hand-over, and every
reference here is evaluated on Context.device_cloud -- the first `points` rows of pos4, the features of feat8, the
caller's index of the row in feat8[:, 5] (tests/cloud_layout_ref.py) --, which device_order() holds to be a permutation of
the caller's rows bit for bit.  The boundaries in question are 64 rows (a wave, a bounding sphere), 256 rows (a tile) and
n_fixed; 300 rows hold all of them.

acvo's row rule.  The Ayy sum of dl counts the rows N <= i < M of the moving cloud AS THE CALLER HANDED IT OVER
(adaptive_cvo.cpp:243-265); the kernels carry the caller's index of every row along (FEAT_INDEX_SLOT) and test that, so a
shard [slo, shi) of device rows sums its members whose caller's index is >= n_fixed -- on the oracle, where the order is
the caller's, exactly the rows [max(slo, n_fixed), shi).  The moving-row cuts at n_fixed - 1, n_fixed, n_fixed + 1 are cuts
of the device rows all the same: the count of a shard's Ayy members is of ALL its rows, its sum of the counted ones.

The partition bound.  The shards' float64 sums are the whole pass's float64 sum of the same float32 terms in another
order; either order is within (N - 1) 2^-53 S of the exact sum of those terms, N the number of members and S the sum of
their absolute values, so |sum_r part_r - whole| <= 2 N 2^-53 S with the reference's S (s_omega, s_v, s_a, s_a_d2,
coeff_scales, each >= the float32 terms' up to 1e-6 relative, which the factor N / (N - 1) covers).  Derived, not fitted.
"""
import threading

import numpy as np

import cvo_iteration_ref as ref
import iteration_ref_cases as ic
import loop_ref_cases as lc
from iteration_ref_judge import Ref, check_flow, check_self

U53 = 2.0 ** -53
SIZES = [(300, 260), (260, 300), (257, 63), (64, 1), (1, 300)]
MATLAB_SIZES = [(300, 260), (257, 63)]
MODES = ["cvo", "acvo", "matlab"]
ACVO_TAIL_SIZE = (260, 300)              # m > n: the Ayy rows that count exist
HOSTILE = [("far600", "cvo", 0.06, 1), ("dup", "acvo", 0.1, 1)]   # (case, mode, ell, index into hostile_cases.poses)
HOSTILE_CUT = "straddle"
BORDER_CAP = 1e-3                        # at most 1 borderline pair per 1 000 members of a record
# (name, mode, setting of loop_ref_cases, size)
LOOP_CASES = [("cvo_300x260", "cvo", "cvo_default", (300, 260)), ("acvo_260x300", "acvo", "acvo_default", (260, 300)),
              ("cvo_257x63", "cvo", "cvo_default", (257, 63))]
NO_EXCHANGE_SHARD = dict(cvo=(65, 257, 0, None), acvo=(65, 257, 64, None))   # (None: the moving cloud's end)


class JudgeFailure(AssertionError):
    def __init__(self, judge, detail):
        super().__init__("%s: %s" % (judge, detail))
        self.judge = judge


def hold(judge, cond, detail=""):
    if not cond:
        raise JudgeFailure(judge, detail() if callable(detail) else detail)


def named(judge, fn, *args, **kw):
    try:
        return fn(*args, **kw)
    except JudgeFailure:
        raise
    except AssertionError as e:
        raise JudgeFailure(judge, e) from None


# ---- the cuts

def even(n, world):
    """cvo_hip_shard_range's split as a cut list."""
    return tuple(n * r // world for r in range(world + 1))


def _mono(n, *inner):
    """(0, inner..., end) with end = n, or the last inner cut where that lies beyond n: cut lists do not decrease."""
    return (0,) + tuple(inner) + (max(n, inner[-1]),)


def cut_lists(n):
    """name -> cut list over n rows."""
    return {"even2": even(n, 2), "even3": even(n, 3), "even4": even(n, 4), "even8": even(n, 8),
            "first_row": _mono(n, 1), "last_row": _mono(n, max(n - 1, 0)),
            "wave": _mono(n, 63, 64, 65), "tile": _mono(n, 255, 256, 257), "straddle": _mono(n, 65, 130),
            "empty_first": (0, 0, n), "empty_last": (0, n, n),
            "hi_clamped": (0, 150, max(n, 150) + 100),     # (the last rank's hi lies beyond n)
            "lo_past_n": (0, n + 5, n + 9)}                # (the second rank is empty by rlo = min(rlo, rhi))


CUT_NAMES = tuple(cut_lists(300))
LOOP_CUT_NAMES = tuple(k for k in CUT_NAMES if k != "even8")   # world <= 4; even8 runs once


def moving_cut_lists(n_fixed, m):
    """acvo, m > n_fixed: the moving-row cuts, chosen apart from the fixed rows' (world 2)."""
    return {"nf-1": (0, n_fixed - 1, m), "nf": (0, n_fixed, m), "nf+1": (0, n_fixed + 1, m), "64": (0, 64, m),
            "even2": even(m, 2)}


def ranges(cuts):
    return [(cuts[r], cuts[r + 1]) for r in range(len(cuts) - 1)]


def clamp(lo, hi, n):
    """cvo_plan.cpp shard_ranges."""
    hi = min(hi, n)
    return min(lo, hi), hi


def shards_of(cuts, mcuts):
    assert len(cuts) == len(mcuts) and all(a <= b for c in (cuts, mcuts) for a, b in zip(c, c[1:])) and cuts[0] == mcuts[0] == 0
    return [f + s for f, s in zip(ranges(cuts), ranges(mcuts))]


# ---- the device's order

def device_order(dc, x, f):
    """(xyz, feat5, ids) of Context.device_cloud's dict: its rows are the caller's rows x, f in another order, bit for bit."""
    n = dc["points"]
    assert n == len(x)
    xyz, feat = np.ascontiguousarray(dc["pos"][:n, :3]), np.ascontiguousarray(dc["feat"][:n, :5])
    ids = np.ascontiguousarray(dc["feat"][:n, 5]).view(np.int32).astype(np.int64)
    b = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)   # noqa: E731
    hold("device_order", np.array_equal(np.sort(ids), np.arange(n)), "the rows' indices are no permutation")
    hold("device_order", np.array_equal(b(xyz), b(np.asarray(x, np.float32)[ids])) and
         np.array_equal(b(feat), b(np.asarray(f, np.float32)[ids])) and
         np.array_equal(b(dc["pos"][:n, 3]), b(feat[:, 4])), "a device row is not the caller's row it names")
    return xyz, feat, ids


# ---- part A: the passes of one shard, and of a partition

class PassStats(dict):
    def count(self, key, v=1):
        self[key] = self.get(key, 0) + v

    def least(self, key, v):
        self[key] = min(self.get(key, v), v)


def _within(judge, got, want, bound, what):
    hold(judge, np.all(np.abs(np.asarray(got) - np.asarray(want)) <= bound), lambda: "%s: %r against %r, bound %r" % (what, got, want, bound))


def judge_passes(pkg, open_ctx, transform, p, mode, clouds, shards, ells, poses_of, worst, stats, steps=True, twist_seed=0):
    """Every shard of `shards` ((lo, hi, slo, shi) as handed to set_shard) and their sum against the references, for the
    length scales `ells` and the poses poses_of(ell) -- module docstring; open_ctx(shard or None) gives the context-like object
    (the library's Context, or OracleContext)."""
    xf, ff, xm, fm = clouds
    n, m = len(xf), len(xm)
    acvo = mode == "acvo"
    whole = open_ctx(None)
    ctxs = [open_ctx(s) for s in shards]
    try:
        dxf, dff, idf = device_order(whole.device_cloud(0), xf, ff)
        dxm, dfm, idm = device_order(whole.device_cloud(1), xm, fm)
        cl = [clamp(s[0], s[1], n) + clamp(s[2], s[3], m) for s in shards]
        # (the partition: the clamped ranges tile [0, n) and [0, m))
        assert sorted(r for c in cl for r in range(c[0], c[1])) == list(range(n))
        assert sorted(r for c in cl for r in range(c[2], c[3])) == list(range(m))
        for ell in ells:
            if acvo:   # function_inner_product: the untransformed clouds, its own cuts; the mean over the shard's own members
                for c, (lo, hi, _, _) in zip(ctxs, cl):
                    got = c.function_inner_product(ell)
                    if hi <= lo:
                        hold("empty", np.isnan(got), "function_inner_product of an empty shard is %r" % got)
                        continue
                    want, _, count, margin = ref.function_inner_product(p, ell, dxf[lo:hi], dff[lo:hi], dxm, dfm)
                    stats.count("borderline", int(ref.classify(margin)[1].sum()))
                    if count == 0:
                        hold("fip", np.isnan(got), got)
                    else:
                        tol = (ic.kw(p) + 1) * ic.U * abs(want)
                        worst.see("fip", abs(got - want), tol)
                        _within("fip", got, want, tol, "function_inner_product rows [%d, %d)" % (lo, hi))
            for _, R, T in poses_of(ell):
                y = transform(R, T, dxm)
                W = Ref(p, ell, dxf, dff, y, dfm)
                stats.count("borderline", len(W.brows))
                stats.count("members", len(W.rows))
                whole.transform_pcd(R, T)
                out_w = whole.flow(ell)
                named("whole", check_flow, out_w, W, worst)
                omega, v = out_w[0:3].astype(np.float32), out_w[3:6].astype(np.float32)
                tw = ([(0.0, omega, v)] + ic.twists(seed=twist_seed)) if steps else []
                bc_w = [whole.step_coeffs(w_, v_, ell) for _, w_, v_ in tw]
                if acvo:
                    Sx, Sy = Ref(p, ell, dxf, dff, dxf, dff), Ref(p, ell, y, dfm, y, dfm, row_ids=idm)
                    stats.count("borderline", len(Sx.brows) + len(Sy.brows))
                sum_f, sum_s = np.zeros(13), [np.zeros(4) for _ in tw]
                for r, (c, (lo, hi, slo, shi)) in enumerate(zip(ctxs, cl)):
                    c.transform_pcd(R, T)
                    out = c.flow(ell)
                    sum_f += out
                    S_ = W.shard(lo, hi)
                    if hi - lo > 2 and (n, m) == SIZES[0] and ell >= 0.06:
                        stats.least("least_members", len(S_.rows))
                    elif hi > lo and (n, m) == SIZES[0] and ell >= 0.06:   # (one or two rows: a single point may have no member at a pose)
                        stats.count("members_of_small_shards", len(S_.rows))
                    if hi <= lo:
                        hold("empty", not np.any(out[0:11]), lambda: "rank %d has no fixed rows and sums %r" % (r, out))
                    if shi <= slo or not acvo:
                        hold("empty", not np.any(out[11:13]), lambda: "rank %d has no moving rows and sums %r" % (r, out))
                    named("shard", check_flow, out, S_, worst)
                    if acvo:
                        named("shard_xx", check_self, out, 9, Sx.shard(lo, hi), 0, worst)
                        named("shard_yy", check_self, out, 11, Sy.shard(slo, shi), n, worst)
                    for k, (_, w_, v_) in enumerate(tw):
                        bcde = c.step_coeffs(w_, v_, ell)
                        sum_s[k] += bcde
                        st, tol = S_.step(w_, v_)
                        worst.see("bcde", np.abs(bcde - st["bcde"]), tol)
                        _within("shard_step", bcde, st["bcde"], tol, "bcde rows [%d, %d)" % (lo, hi))
                        if hi <= lo:
                            hold("empty", not np.any(bcde), lambda: "rank %d has no rows and bcde %r" % (r, bcde))
                # the partition: counts exactly, sums to the bound of two summation orders
                for k in (8, 10, 12):
                    hold("partition_count", int(sum_f[k]) == int(out_w[k]), lambda: "out[%d]: the shards have %d, the whole %d" % (k, sum_f[k], out_w[k]))
                fl = W.flow()[0]
                nb = 2.0 * len(W.rows) * U53
                for sl, key in ((slice(0, 3), "s_omega"), (slice(3, 6), "s_v"), (slice(6, 7), "s_a"), (slice(7, 8), "s_a_d2")):
                    worst.see("partition", np.abs(sum_f[sl] - out_w[sl]), nb * np.asarray(fl[key]))
                    _within("partition_sum", sum_f[sl], out_w[sl], nb * np.asarray(fl[key]), key)
                if acvo:
                    for k, S_, first in ((9, Sx, 0), (11, Sy, n)):
                        b = 2.0 * len(S_.rows) * U53 * S_.self_flow(first)["s_a_d2"]
                        worst.see("partition", abs(sum_f[k] - out_w[k]), b)
                        _within("partition_sum", sum_f[k], out_w[k], b, "out[%d]" % k)
                for k, (_, w_, v_) in enumerate(tw):
                    b = nb * W.step(w_, v_)[0]["coeff_scales"]
                    worst.see("partition", np.abs(sum_s[k] - bc_w[k]), b)
                    _within("partition_sum", sum_s[k], bc_w[k], b, "bcde")
    finally:
        for c in ctxs + [whole]:
            c.close()


# ---- the oracle behind the calls of a Context (rows in the caller's order: its device order is the identity)

class OracleContext:
    """What judge_passes calls on a Context, made of the oracle's own passes over the rows of a shard.  ayy_first: the first
    row the Ayy sum counts (n_fixed; 0 is the driver's error MUTANT_AYY)."""

    def __init__(self, po, p, mode, clouds, shard=None, ayy_first=None):
        self.po, self.p, self.mode = po, p, mode
        self.xf, self.ff, self.xm, self.fm = (np.ascontiguousarray(a, np.float32) for a in clouds)
        n, m = len(self.xf), len(self.xm)
        lo, hi, slo, shi = shard if shard is not None else (0, n, 0, m)
        self.lo, self.hi = clamp(lo, hi, n)
        self.slo, self.shi = clamp(slo, shi if shi is not None else m, m)
        self.search = po.SEARCH_DENSE if mode == "matlab" else po.SEARCH_GRID
        self.ayy_first = n if ayy_first is None else ayy_first
        self.y = self.xm

    def device_cloud(self, which):
        x, f = (self.xf, self.ff) if which == 0 else (self.xm, self.fm)
        n = len(x)
        feat = np.zeros((n, 8), np.float32)
        feat[:, :5] = f
        feat[:, 5] = np.arange(n, dtype=np.int32).view(np.float32)
        return dict(pos=np.concatenate([x, f[:, 4:5]], axis=1), feat=feat, points=n, rows=n)

    def transform_pcd(self, R, T):
        self.y = self.po.transform(R, T, self.xm)

    def _xy(self, ell):
        return self.po.se_kernel(self.p, ell, self.xf[self.lo:self.hi], self.ff[self.lo:self.hi], self.y, self.fm, search=self.search)

    def flow(self, ell):
        po, p, out = self.po, self.p, np.zeros(13)
        if self.hi > self.lo:
            csr = self._xy(ell)
            om, v, sa, sad2 = po.flow(p, ell, self.xf[self.lo:self.hi], self.y, csr)
            out[0:3], out[3:6], out[6], out[7], out[8] = om, v, sa, sad2, csr[0][-1]
        if self.mode == "acvo":
            if self.hi > self.lo:
                xa, fa = self.xf[self.lo:self.hi], self.ff[self.lo:self.hi]
                csr = po.se_kernel(p, ell, xa, fa, self.xf, self.ff, search=self.search)
                out[9], out[10] = po.flow(p, ell, xa, self.xf, csr)[3], csr[0][-1]
            if self.shi > self.slo:
                ya, fa = self.y[self.slo:self.shi], self.fm[self.slo:self.shi]
                rp, col, val = po.se_kernel(p, ell, ya, fa, self.y, self.fm, search=self.search)
                out[12] = rp[-1]
                first = max(self.ayy_first - self.slo, 0)          # (local rows below it do not count)
                if first < len(ya):
                    rp2 = (rp - rp[first]).clip(min=0)
                    out[11] = po.flow(p, ell, ya, self.y, (rp2, col[rp[first]:].copy(), val[rp[first]:].copy()))[3]
        return out

    def step_coeffs(self, omega, v, ell):
        if self.hi <= self.lo:
            return np.zeros(4)
        return self.po.step_coeffs(ell, omega, v, self.xf[self.lo:self.hi], self.y, self._xy(ell))

    def function_inner_product(self, ell):
        if self.hi <= self.lo:
            return float("nan")
        return self.po.function_inner_product(self.p, ell, self.xf[self.lo:self.hi], self.ff[self.lo:self.hi], self.xm, self.fm,
                                              search=self.search)

    def close(self):
        pass


# Mutants of the driver of part A: what a driver with one plausible error hands to set_shard for rank r of `shards` (n, m:
# the clouds' sizes).  "ayy": the Ayy rule applied from row 0.
def _m_shift(dlo, dhi, rank):
    def f(shards, r, n, m):
        lo, hi, slo, shi = shards[r]
        return (max(lo + dlo, 0), max(hi + dhi, lo + dlo, 0), slo, shi) if r == rank else shards[r]
    return f


MUTANT_SHARDS = {
    "rows [lo + 1, hi)": _m_shift(1, 0, 1),
    "rows [lo, hi - 1)": _m_shift(0, -1, 0),
    "rows [lo - 1, hi), overlapping the neighbour": _m_shift(-1, 0, 1),
    "the shard ignored on one rank": lambda shards, r, n, m: (0, n, 0, m) if r == 1 else shards[r],
    "the moving-row cut taken from the fixed-row cut": lambda shards, r, n, m: shards[r][:2] + shards[r][:2],
}
MUTANT_AYY = "Ayy rows counted from 0 instead of n_fixed"


# ---- part B: whole registrations of several ranks.  run_ranks(p, shards, trace_cap) -> [dict per rank: n_it, raw (the
# state's bytes), state0, state1 (loop_ref_cases.snap), trace, calls, stats (Context.list_stats() or None)];
# run_whole(p) -> the same dict of the unsharded registration.

def host_sum_ranks(world, timeout):
    """The all-reduce of `world` host threads around a barrier with a time-out: (reduce(r, mine) -> the sum in rank order, the
    barrier).  A rank that does not come ends its peers' wait as threading.BrokenBarrierError after `timeout` seconds."""
    barrier = threading.Barrier(world, timeout=timeout)
    box = [None] * world

    def reduce(r, mine):
        box[r] = np.array(mine, np.float64)
        barrier.wait()
        total = box[0].copy()
        for q in range(1, world):
            total = total + box[q]
        barrier.wait()
        return total
    return reduce, barrier


def oracle_ranks(po, mode, clouds, timeout=20.0, mutant=None):
    """run_ranks over the oracle's sharded loop (cvo_oracle_align_sharded), one host thread per rank.  mutant: "twice" (rank
    1's partials enter the sum twice), "skip_step" (rank 1's step partials are left out of the second exchange),
    "empty_skips" (a rank without rows takes no part in the exchanges)."""
    xf, ff, xm, fm = clouds
    n, m = len(xf), len(xm)
    search = po.SEARCH_DENSE if mode == "matlab" else po.SEARCH_GRID

    def one_thread(fn):
        # (the oracle's OpenMP reductions add their threads' partial sums in the order the threads arrive: with one thread per
        # rank its float64 sums are the same bits in every run, which the prefix judge needs)
        def wrapped(*a, **kw):
            before = po.get_threads()
            po.set_threads(1)
            try:
                return fn(*a, **kw)
            finally:
                po.set_threads(before)
        return wrapped

    @one_thread
    def run_ranks(p, shards, trace_cap=2000):
        world = len(shards)
        reduce, barrier = host_sum_ranks(world, timeout)
        out, errors = [None] * world, []

        def rank(r):
            lo, hi, slo, shi = shards[r]
            lo, hi = clamp(lo, hi, n)
            slo, shi = clamp(slo, shi, m)
            calls = [0]
            broken = []

            def allreduce(arr):
                calls[0] += 1
                if broken or (mutant == "empty_skips" and hi <= lo and shi <= slo):
                    return
                try:
                    mine = arr.copy()
                    if r == 1 and mutant == "twice":
                        mine = 2.0 * mine
                    if r == 1 and mutant == "skip_step" and len(arr) == 4:
                        mine[:] = 0.0
                    arr[:] = reduce(r, mine)
                except threading.BrokenBarrierError:
                    broken.append(1)
                    errors.append((r, "a peer did not come to exchange %d within %g s" % (calls[0], timeout)))
            try:
                st = po.init_state(p)
                s0 = lc.snap(st)
                n_it, tr = po.align(p, st, xf, ff, xm, fm, search=search, trace_cap=max(trace_cap, 1), shard=(lo, hi, slo, shi),
                                    allreduce=allreduce)
                out[r] = dict(n_it=n_it, raw=bytes(st), state0=s0, state1=lc.snap(st), trace=tr[:trace_cap], calls=calls[0], stats=None)
            except Exception as e:   # pragma: no cover
                errors.append((r, repr(e)))
                barrier.abort()
        ts = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=10 * timeout)
        hold("barrier", not errors, lambda: errors[:3])
        hold("barrier", all(o is not None for o in out), "a rank did not finish")
        return out

    @one_thread
    def run_whole(p, shard=None, trace_cap=2000):
        st = po.init_state(p)
        s0 = lc.snap(st)
        n_it, tr = po.align(p, st, xf, ff, xm, fm, search=search, trace_cap=max(trace_cap, 1), shard=shard)
        return dict(n_it=n_it, raw=bytes(st), state0=s0, state1=lc.snap(st), trace=tr[:trace_cap], calls=0, stats=None)
    return run_ranks, run_whole


def same_trace(a, b):
    """Two traces record for record, every field, bit for bit."""
    def eq(x, y):
        return np.array_equal(np.asarray(x, np.float64), np.asarray(y, np.float64), equal_nan=True)
    return len(a) == len(b) and all(x.keys() == y.keys() and all(eq(x[k], y[k]) for k in x) for x, y in zip(a, b))


def judge_lock_step(pkg, ranks, whole):
    """All ranks bit-identical in state and trace, the same number of exchanges on every rank (an empty one included), the
    unsharded registration's iteration count, its transform within 1e-6."""
    r0 = ranks[0]
    for r, o in enumerate(ranks):
        hold("lock_step", o["raw"] == r0["raw"] and o["n_it"] == r0["n_it"], "rank %d left lock step: its state differs" % r)
        hold("lock_step", same_trace(o["trace"], r0["trace"]), "rank %d left lock step: its trace differs" % r)
        hold("hook_calls", o["calls"] == r0["calls"], lambda: "exchanges per rank: %r" % [q["calls"] for q in ranks])
    hold("iterations", r0["n_it"] == whole["n_it"], lambda: "sharded %d, unsharded %d iterations" % (r0["n_it"], whole["n_it"]))
    rot, tra = pkg.data.rel_pose_error(r0["state1"]["transform"], whole["state1"]["transform"])
    hold("transform", rot <= 1e-6 and tra <= 1e-6, lambda: "against the unsharded registration: rot %g, trans %g" % (rot, tra))


def judge_replay(p, run, worst=None, census=None):
    bad = lc.judge_run(dict(p=p, state0=run["state0"], trace=run["trace"], n_it=run["n_it"], state1=run["state1"]), worst=worst,
                       census=census)
    hold("replay", not bad, lambda: bad[:4])


def judge_record(p, mode, t, pose, dev, transform, worst, stats, with_dl=False, rows=None):
    """One trace record against the dense reference at the exact pose it was formed at (pose: the state of the run one
    iteration shorter).  dev: ((dxf, dff, idf), (dxm, dfm, idm)).  rows: (lo, hi, slo, shi) of a shard without an exchange."""
    (dxf, dff, idf), (dxm, dfm, idm) = dev
    n, m = len(dxf), len(dxm)
    lo, hi, slo, shi = rows if rows is not None else (0, n, 0, m)
    ell = np.float32(t["ell"])
    y = transform(pose["R"], pose["T"], dxm)
    W = Ref(p, ell, dxf, dff, y, dfm).shard(lo, hi)
    stats.count("records")
    stats.count("record_members", len(W.rows))
    hold("borderline_cap", len(W.brows) <= BORDER_CAP * len(W.rows),
         lambda: "record %d: %d borderline pairs among %d members" % (t["k"], len(W.brows), len(W.rows)))
    hold("record_count", W.count_ok(t["nnz"]), lambda: "record %d: nnz %d, the reference has %d (+%d borderline)" % (t["k"], t["nnz"], W.sure_in, len(W.brows)))
    fl, tol = W.flow()
    for key in ("omega_d", "v_d", "sum_a"):
        worst.see(key, np.abs(np.asarray(t[key]) - fl[key]), tol[key])
        _within("record_flow", t[key], fl[key], tol[key], "record %d %s" % (t["k"], key))
    stp, stol = W.step(np.array(t["omega"], np.float32), np.array(t["v"], np.float32))
    worst.see("bcde", np.abs(np.array(t["bcde"]) - stp["bcde"]), stol)
    _within("record_step", t["bcde"], stp["bcde"], stol, "record %d bcde" % t["k"])
    if mode == "acvo":
        Sx, Sy = Ref(p, ell, dxf, dff, dxf, dff).shard(lo, hi), Ref(p, ell, y, dfm, y, dfm, row_ids=idm).shard(slo, shi)
        hold("record_count", Sx.count_ok(t["nnz_xx"]) and Sy.count_ok(t["nnz_yy"]),
             lambda: "record %d: nnz_xx %d (%d), nnz_yy %d (%d)" % (t["k"], t["nnz_xx"], Sx.sure_in, t["nnz_yy"], Sy.sure_in))
        if with_dl:
            hold("borderline_cap", len(W.brows) + len(Sx.brows) + len(Sy.brows) == 0, "a borderline pair in a record held to dl")
            # (cvo_iteration_ref.dl applies the row rule to the rows it is given: the caller's indices)
            d = ref.dl(ell, dxf[np.argsort(idf)], y[np.argsort(idm)], (idf[W.rows], idm[W.cols], W.am),
                       (idf[Sx.rows], idf[Sx.cols], Sx.am), (idm[Sy.rows], idm[Sy.cols], Sy.am))
            worst.see("dl", abs(t["dl"] - d["dl"]), ic.dl_tol(p, d))
            _within("record_dl", t["dl"], d["dl"], ic.dl_tol(p, d), "record %d dl" % t["k"])


def census_of(chain, stats):
    """How many of the judged records streamed a list made earlier and how many followed a narrowing of the record: from
    Context.list_stats() of the runs one iteration apart where the driver has it ((builds, narrowings, re-expansions) of a
    registration), else from ell between records -- a drop of ell narrows, an unchanged ell re-uses."""
    for j in range(1, len(chain)):
        a, b = chain[j - 1], chain[j]
        if b["n_it"] != j or not b["trace"]:
            continue
        if b["stats"] is not None and a["stats"] is not None and j > 1:
            grew = [y - x for x, y in zip(a["stats"], b["stats"])]
            stats.count("after_narrowing", int(grew[1] > 0))
            stats.count("on_reused_list", int(not any(grew)))
        elif j > 1:
            e0, e1 = np.float32(b["trace"][j - 2]["ell"]), np.float32(b["trace"][j - 1]["ell"])
            stats.count("after_narrowing", int(e1 < e0))
            stats.count("on_reused_list", int(e1 == e0))


def judge_sharded_registration(pkg, api, run_ranks, run_whole, dev, transform, mode, name, shards, worst, stats, prefixes=True):
    """The judges of a whole registration over `shards`: lock step and the unsharded result, the replay of rank 0's trace, and
    (prefixes) every record of the runs with max_iter = 0 ... J against the dense reference at its exact pose."""
    over = lc.setting(name)[2]
    p = lc.params(api, mode, over)
    full = run_ranks(p, shards)
    whole = run_whole(p)
    judge_lock_step(pkg, full, whole)
    stats.count("hook_calls", full[0]["calls"])
    stats.count("registrations")
    judge_replay(p, full[0], worst=worst)
    if not prefixes:
        return full
    J = lc.PREFIX_J[mode]
    chain = []
    for j in range(J + 1):
        pj = lc.params(api, mode, dict(over, max_iter=j))
        rk = run_ranks(pj, shards)
        judge_lock_step(pkg, rk, run_whole(pj))
        hold("prefix", rk[0]["n_it"] == min(j, full[0]["n_it"]), lambda: "max_iter %d ran %d iterations" % (j, rk[0]["n_it"]))
        chain.append(rk[0])
    judge_chain(p, mode, full[0], chain, dev, transform, worst, stats)
    return full


def judge_chain(p, mode, full, chain, dev, transform, worst, stats):
    """chain[j]: rank 0's run with max_iter = j, j = 0 ... J; full: its whole registration.  Every run is a bit-identical prefix
    of the next and of the full one, so the state of run j is the exact pose at which record j was formed: record j is held
    there against the dense reference; and the census of the records between two runs (census_of)."""
    J = len(chain) - 1
    for j in range(1, J + 1):
        hold("prefix", lc.same_records(chain[j - 1]["trace"], chain[j]["trace"][:j - 1]) and
             same_trace(chain[j - 1]["trace"], chain[j]["trace"][:j - 1]), "the run with max_iter %d is no prefix of the next" % (j - 1))
    hold("prefix", same_trace(chain[J]["trace"], full["trace"][:J]), "the run with max_iter %d is no prefix of the full one" % J)
    for j in range(min(J, full["n_it"] - 1) + 1):
        judge_record(p, mode, full["trace"][j], chain[j]["state1"], dev, transform, worst, stats, with_dl=(j == 0))
    census_of(chain, stats)


def judge_no_exchange(pkg, api, run_whole, dev, transform, mode, name, rows, worst, stats):
    """A shard without an exchange: record 0 of max_iter = 1 against the reference's members of those rows (nnz equal, no
    borderline pair; sums, step coefficients and for acvo the counts and dl of the three restricted member sets), and the
    full run through the replay judge.  run_whole(p, shard=rows) is the driver.  Returns the full run."""
    over = lc.setting(name)[2]
    p1 = lc.params(api, mode, dict(over, max_iter=1))
    one = run_whole(p1, shard=rows)
    hold("iterations", one["n_it"] == 1 and len(one["trace"]) == 1, one["n_it"])
    n, m = len(dev[0][0]), len(dev[1][0])
    cl = clamp(rows[0], rows[1], n) + clamp(rows[2], rows[3], m)
    judge_record(p1, mode, one["trace"][0], one["state0"], dev, transform, worst, stats, with_dl=(mode == "acvo"), rows=cl)
    W = Ref(p1, np.float32(one["trace"][0]["ell"]), dev[0][0], dev[0][1], transform(one["state0"]["R"], one["state0"]["T"], dev[1][0]),
            dev[1][1]).shard(cl[0], cl[1])
    hold("record_count", len(W.brows) == 0 and one["trace"][0]["nnz"] == len(W.rows) > 0,
         lambda: "record 0: nnz %d, the reference's rows [%d, %d) hold %d" % (one["trace"][0]["nnz"], cl[0], cl[1], len(W.rows)))
    p = lc.params(api, mode, over)
    full = run_whole(p, shard=rows)
    judge_replay(p, full, worst=worst)
    return full
