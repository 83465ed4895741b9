"""GPU: how a registration begins and ends inside an engine of cvo_hip_align_many (csrc/cvo_engine.cpp).

The registrations an engine takes in one pump are prepared by ONE launch (k_prepare_many, a block each, MAXG per launch), the
table's build masks are armed once, and a registration that stops with a verdict is handed back from the pinned copy of its final
head (the post-step kernel writes it in front of the `done` word) instead of a copy of the whole state behind the queued batches.
None of this may change what a registration computes: every case compares the iteration counts and the bytes of the final
states of an align_many call with cvo_hip_align of the same pair on the same context (the rule of
test_headline_shape_64_distinct_10k_pairs_through_the_engines).  The contexts' read-only counters say that the call really went
through the engines ("engine_begins") and which way its states came back ("engine_final_mirrored", "engine_final_copied").

Clouds are a few hundred points (the overflow case: 1 500): more than 12 registrations per call, or the call would leave them to their own streams
(better_alone)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _far_state(capi, p):
    """A start well off the identity: the registration travels for many iterations."""
    st = capi.init_state(p)
    a = 0.06
    R = [np.cos(a), -np.sin(a), 0.0, np.sin(a), np.cos(a), 0.0, 0.0, 0.0, 1.0]
    for q in range(9):
        st.R[q] = np.float32(R[q])
    for q, v in enumerate((0.12, -0.08, 0.05)):
        st.T[q] = np.float32(v)
    return st


def _contexts(pkg, mode, count, points, options=(), max_iters=None, blob=False):
    """`count` contexts with distinct pairs of points + 7 b points (odd sizes, no two alike).  blob: the clouds shrunk until
    every point is within reach of every other (tests/hostile_cases.py "blob"): with the lists started at their minimum
    ("list_init") the kept list overflows in the first iterations."""
    import torch
    capi = pkg.capi
    acvo = mode == capi.MODE_ACVO
    ctxs, streams = [], []
    for b in range(count):
        n = points + 7 * b
        xf, ff, xm, fm = pkg.data.synthetic_pair(n, n - 3, seed=pkg.data.SEED_CFG5_BASE + 100 + b, acvo=acvo)
        if blob:
            xf = (xf.astype(np.float64) * 0.08 + np.array([0.0, 0.0, 1.2])).astype(np.float32)
            xm = (xm.astype(np.float64) * 0.08 + np.array([0.0, 0.0, 1.2])).astype(np.float32)
        s = torch.cuda.Stream()
        p = capi.default_params(mode)
        if max_iters is not None and max_iters[b % len(max_iters)] is not None:
            p.max_iter = max_iters[b % len(max_iters)]
        c = capi.Context(params=p, device=0, stream=s.cuda_stream, graph_capture=True)
        for key, value in options:
            c.set_option(key, value)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        ctxs.append(c); streams.append(s)
    return ctxs, streams


def _counters(ctxs):
    return {k: int(sum(c.get_option(k) for c in ctxs))
            for k in ("engine_begins", "engine_final_mirrored", "engine_final_copied", "tail_handovers", "list_grows")}


def _many_equals_alone(pkg, ctxs, far=(), calls=2):
    """align_many (twice: the second call re-uses the engines' tables and captured batches), then every pair on its own."""
    capi = pkg.capi
    first = lambda b, c: _far_state(capi, c.params) if b in far else capi.init_state(c.params)
    before = _counters(ctxs)
    for _ in range(calls):
        states = [first(b, c) for b, c in enumerate(ctxs)]
        its = capi.align_many(ctxs, states)
    after = _counters(ctxs)
    moved = {k: after[k] - before[k] for k in after}
    print("iterations", list(its), "counters", moved)
    for b, c in enumerate(ctxs):
        st = first(b, c)
        n_l, _ = c.align(st, trace_cap=0)
        assert n_l == its[b], (b, n_l, its[b])
        assert bytes(st) == bytes(states[b]), b
    return its, moved


def _close(ctxs):
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_24_pairs_in_one_engine_fill_more_than_one_group(pkg, mode_name):
    """24 registrations begin in ONE engine ("engines" = 1): its first pump prepares 24 entries, one group of MAXG = 16 and one
    of 8."""
    capi = pkg.capi
    mode = capi.MODE_CVO if mode_name == "cvo" else capi.MODE_ACVO
    ctxs, streams = _contexts(pkg, mode, 24, 400, options=(("engines", 1),))
    try:
        its, moved = _many_equals_alone(pkg, ctxs)
        assert moved["engine_begins"] >= 2 * 24                      # every registration of both calls began in an engine
        assert moved["engine_final_mirrored"] + moved["engine_final_copied"] + moved["tail_handovers"] >= 2 * 24
        assert moved["engine_final_mirrored"] >= 24                  # ... and the engines handed states back from the pinned heads
        assert len(set(its)) > 3
    finally:
        _close(ctxs)


def test_40_pairs_share_the_32_slots_of_one_engine(pkg):
    """More registrations than slots: the last eight begin in later pumps, in slots that fell free while batches were queued,
    and the first ones are handed back through their pinned heads while the engine runs on."""
    capi = pkg.capi
    ctxs, streams = _contexts(pkg, capi.MODE_CVO, 40, 300, options=(("engines", 1),))
    try:
        its, moved = _many_equals_alone(pkg, ctxs)
        assert moved["engine_begins"] >= 2 * 40
        assert moved["engine_final_mirrored"] >= 40
    finally:
        _close(ctxs)


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_mixed_max_iter_in_one_call(pkg, mode_name):
    """max_iter 0 (nothing to run: the state comes back by a copy behind the registration's prepare), 1, 25 and the default in
    one call."""
    capi = pkg.capi
    mode = capi.MODE_CVO if mode_name == "cvo" else capi.MODE_ACVO
    ctxs, streams = _contexts(pkg, mode, 20, 350, max_iters=(0, 1, 25, None))
    try:
        its, moved = _many_equals_alone(pkg, ctxs)
        assert moved["engine_begins"] >= 2 * 20
        for b in range(20):
            want = (0, 1, 25, None)[b % 4]
            if want is not None:
                assert its[b] <= want, (b, its[b])
            if want == 0:
                assert its[b] == 0
        assert moved["engine_final_mirrored"] >= 10
    finally:
        _close(ctxs)


@pytest.mark.parametrize("tail_alone", [8, 0])
def test_lists_that_overflow_inside_the_engines(pkg, tail_alone):
    """Every list starts at its minimum capacity ("list_init") and the clouds are blobs: the registrations park with
    NEED_BIGGER_LIST, come back by the copy of the whole state (the host needs the counters of its tail), grow their lists and
    resume through the batched prepare -- with the call's tail leaving the engines ("tail_alone" 8) and without.  (1 500 points, the
    size of tests/hostile_cases.py's blob: the kept list's minimum holds 262 144 members, fewer points cannot overflow it.)"""
    capi = pkg.capi
    ctxs, streams = _contexts(pkg, capi.MODE_CVO, 16, 1500, options=(("list_init", 1), ("tail_alone", tail_alone)), blob=True)
    try:
        its, moved = _many_equals_alone(pkg, ctxs, calls=1)
        assert moved["list_grows"] >= 1
        assert moved["engine_final_copied"] >= 1                     # the parked ones
        assert moved["engine_begins"] > 16                           # ... began a second time
        if tail_alone == 0:
            assert moved["tail_handovers"] == 0
        # the lists have grown: a second call overflows nothing and every state comes back through its pinned head or its tail
        its2, moved2 = _many_equals_alone(pkg, ctxs, calls=1)
        assert list(its2) == list(its)
        assert moved2["list_grows"] == 0 and moved2["engine_final_mirrored"] >= 1
    finally:
        _close(ctxs)


def test_the_tail_leaves_the_engines(pkg):
    """16 registrations, one from a far start: it runs long after the others have stopped and leaves its engine for resident
    runs of its own ("tail_alone" at its default); the leavers' states equal the registrations on their own too."""
    capi = pkg.capi
    ctxs, streams = _contexts(pkg, capi.MODE_CVO, 16, 500)
    try:
        its, moved = _many_equals_alone(pkg, ctxs, far=(5,))
        assert moved["engine_begins"] >= 2 * 16
        assert moved["tail_handovers"] >= 1
    finally:
        _close(ctxs)
