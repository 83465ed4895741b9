"""GPU: narrowing of the candidate record (option `record_narrow`, csrc/cvo_device.h plan_lists).

When the length scale drops the synchronous plan no longer throws a record that is still valid away with its tile list: the
iteration's streaming flow pass writes the candidates inside the new radius back in place.  Membership of A is decided by the
exact test on every candidate in every pass, so nothing a registration computes may change: iteration counts, whole states and
the members per iteration with the option on equal those with it off, those of the registration on its own, and the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _seed(pkg, b):
    return pkg.data.SEED_CFG2 if b == 0 else pkg.data.SEED_CFG5_BASE + b   # (bench.py's pairs)


def _contexts(pkg, mode, count, points, max_iters=None):
    import torch
    capi = pkg.capi
    acvo = mode == capi.MODE_ACVO
    ctxs, streams = [], []
    for b in range(count):
        pr = pkg.data.synthetic_pair(points, points, seed=_seed(pkg, b), acvo=acvo)
        s = torch.cuda.Stream()
        p = capi.default_params(mode)
        if max_iters:
            p.max_iter = max_iters[b % len(max_iters)]
        c = capi.Context(params=p, device=0, stream=s.cuda_stream, graph_capture=True)
        c.set_fixed(pr[0], pr[1])
        c.set_moving(pr[2], pr[3])
        ctxs.append(c); streams.append(s)
    return ctxs, streams


def _align_many(capi, ctxs, narrow, reps=1):
    for c in ctxs:
        c.set_option("record_narrow", narrow)
    for _ in range(reps):
        states = [capi.init_state(c.params) for c in ctxs]
        its = capi.align_many(ctxs, states)
    return its, states, [c.list_stats() for c in ctxs]


def _compare_batched(pkg, mode, count, points, max_iters=None):
    capi = pkg.capi
    ctxs, streams = _contexts(pkg, mode, count, points, max_iters)
    # (two calls each: the second re-uses the engines' captured batches and tables)
    its_on, st_on, stats_on = _align_many(capi, ctxs, 1, reps=2)
    its_off, st_off, stats_off = _align_many(capi, ctxs, 0, reps=2)
    print("mode %d, %d x %dk: builds on/off %d/%d, narrowings on/off %d/%d, re-expansions on/off %d/%d" % (
        mode, count, points // 1000, sum(s[0] for s in stats_on), sum(s[0] for s in stats_off), sum(s[1] for s in stats_on),
        sum(s[1] for s in stats_off), sum(s[2] for s in stats_on), sum(s[2] for s in stats_off)))
    assert list(its_on) == list(its_off)
    for b in range(count):
        assert bytes(st_on[b]) == bytes(st_off[b]), b
    for b, c in enumerate(ctxs):   # ... and the same pair registered on its own (the rule of test_headline_shape_64...)
        c.set_option("record_narrow", 1)
        st = capi.init_state(c.params)
        n_l, _ = c.align(st, trace_cap=0)
        assert n_l == its_on[b], (b, n_l, its_on[b])
        assert bytes(st) == bytes(st_on[b]), b
    for c in ctxs:
        c.close()
    return its_on, stats_on, stats_off


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_24_distinct_6k_pairs_narrowed_equal_rebuilt(pkg, mode_name):
    capi = pkg.capi
    mode = capi.MODE_CVO if mode_name == "cvo" else capi.MODE_ACVO
    _, stats_on, stats_off = _compare_batched(pkg, mode, 24, 6000)
    assert all(s[1] == 0 for s in stats_off)
    if mode_name == "cvo":   # (its schedule drops the length scale by 1.5 and more at a time)
        assert sum(s[1] for s in stats_on) > 0


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_64_distinct_10k_pairs_narrowed_equal_rebuilt(pkg, mode_name):
    """The shape bench.py's `value` is quoted on.  Counters: with the option on the all-pairs builds of the cvo registrations fall
    (4.2 per registration of this set without it, 2.2 with it: DESIGN 4.1) and there are narrowings; with it off there are none."""
    capi = pkg.capi
    mode = capi.MODE_CVO if mode_name == "cvo" else capi.MODE_ACVO
    _, stats_on, stats_off = _compare_batched(pkg, mode, 64, 10000)
    assert all(s[1] == 0 for s in stats_off)
    if mode_name == "cvo":
        assert sum(s[1] for s in stats_on) > 0
        assert sum(s[0] for s in stats_on) < sum(s[0] for s in stats_off)


def test_geometry_changes_after_a_narrowing(pkg):
    """Registrations that stop after 25 / 60 / 200 iterations mixed in one call: the engines change geometry as their slots fall
    free, the flow pass expands the (old, wide) tile list again behind a narrowed record."""
    capi = pkg.capi
    _, stats_on, stats_off = _compare_batched(pkg, capi.MODE_CVO, 24, 6000, max_iters=(25, 60, 200))
    assert all(s[1] == 0 for s in stats_off)
    assert sum(s[1] for s in stats_on) > 0
    assert sum(s[2] for s in stats_on) > 0   # re-expansions ran with the option on


def _far_state(mod, p):
    """A start well off the identity: the first iterations travel far."""
    st = mod.init_state(p)
    a = 0.06
    R = [np.cos(a), -np.sin(a), 0.0, np.sin(a), np.cos(a), 0.0, 0.0, 0.0, 1.0]
    for q in range(9):
        st.R[q] = np.float32(R[q])
    for q, v in enumerate((0.12, -0.08, 0.05)):
        st.T[q] = np.float32(v)
    return st


@pytest.mark.parametrize("mode_name,margin,far", [("cvo", None, False), ("cvo", 0.05, False), ("cvo", None, True),
                                                  ("cvo", 0.05, True), ("acvo", None, False), ("acvo", 0.05, True)])
def test_members_per_iteration_of_a_large_pair(pkg, po, mode_name, margin, far):
    """A 15k x 15k pair is above the sizes of the double-buffered lone plan and below 65 536 rows: it runs through the synchronous
    plan on its own, keeps a candidate record and takes a trace.  The members of A in EVERY iteration with the option on equal
    those with it off and the oracle's -- a narrowed record lost no member.  list_margin 0.05 leaves a narrowing little room
    (the "build instead" branch), the far start travels enough to rebuild after a narrowing."""
    import torch
    capi = pkg.capi
    mode = capi.MODE_CVO if mode_name == "cvo" else capi.MODE_ACVO
    n = 15000
    xf, ff, xm, fm = pkg.data.synthetic_pair(n, n, seed=pkg.data.SEED_CFG5_BASE + 3, acvo=mode_name == "acvo")
    s = torch.cuda.Stream()
    c = capi.Context(mode=mode, device=0, stream=s.cuda_stream, graph_capture=True)
    c.set_fixed(xf, ff)
    c.set_moving(xm, fm)
    if margin is not None:
        c.set_option("list_margin", margin)
    runs = {}
    for narrow in (1, 0):
        c.set_option("record_narrow", narrow)
        st = _far_state(capi, c.params) if far else capi.init_state(c.params)
        n_it, tr = c.align(st, trace_cap=2000)
        runs[narrow] = (n_it, bytes(st), [t["nnz"] for t in tr], c.list_stats())
        print("%s margin %s far %d narrow %d: %d iterations, builds / narrowings / re-expansions %s" % (
            mode_name, margin, far, narrow, n_it, runs[narrow][3]))
    c.close()
    assert runs[1][0] == runs[0][0]
    assert runs[1][2] == runs[0][2]
    assert runs[1][1] == runs[0][1]
    assert runs[0][3][1] == 0
    if mode_name == "cvo" and margin is None and not far:
        assert runs[1][3][1] > 0 and runs[1][3][0] < runs[0][3][0]
    p = po.default_params(po.MODE_CVO if mode_name == "cvo" else po.MODE_ACVO)
    so = _far_state(po, p) if far else po.init_state(p)
    n_or, tr_or = po.align(p, so, xf, ff, xm, fm, search=po.SEARCH_GRID, trace_cap=2000)
    assert n_or == runs[1][0]
    assert [t["nnz"] for t in tr_or] == runs[1][2]
