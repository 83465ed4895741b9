"""GPU: an engine's xy tile lists rebuilt from their candidate records when the launch geometry changes (option
`tiles_from_record`, csrc/cvo_kernels.hip kt_tiles_from_record, csrc/cvo_engine.cpp Engine::replan).

With the option on the slots of an engine narrow their record at every drop of the length scale, and when members leave and the
launches change geometry each remaining slot's tile list is written anew from its record before the flow pass expands it again.
A rebuilt list is the record's own pair set and membership of A is the exact test's on every candidate, so nothing a registration
computes may change: iteration counts and whole states with the option on equal those with it off and those of each pair
registered on its own, byte for byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_ITERS = (25, 60, 200)   # mixed in one call: the engines change geometry as their slots fall free
_LONE = {}                  # (set name) -> [(iterations, state bytes)] of every pair registered on its own


def _seed(pkg, b):
    return pkg.data.SEED_CFG2 if b == 0 else pkg.data.SEED_CFG5_BASE + b   # (bench.py's pairs)


def _surface_pairs(pkg, count, points, acvo):
    return [pkg.data.synthetic_pair(points, points, seed=_seed(pkg, b), acvo=acvo) for b in range(count)]


def _cluster_pairs(count, points):
    """Both clouds: three tight clusters (sigma 8 mm) around the same three centres, the moving one displaced by a few millimetres
    and a small turn.  At the first length scales every pair of a cluster is a candidate -- tile entries with all 64 bits set --
    while the clusters' fringes leave entries with a single bit; a wave's slice of the record ends wherever its count says."""
    out = []
    centres = np.array([[-0.35, -0.2, 1.4], [0.4, -0.1, 1.6], [0.05, 0.35, 1.5]])
    colours = np.array([[40.0, 90.0, 200.0, 3.0, -2.0], [180.0, 60.0, 50.0, -4.0, 1.0], [90.0, 200.0, 120.0, 2.0, 5.0]])
    for b in range(count):
        rng = np.random.Generator(np.random.PCG64(7100 + b))
        clouds = []
        for _ in range(2):
            which = np.arange(points) % 3
            xyz = centres[which] + 0.008 * rng.standard_normal((points, 3))
            feat = colours[which] + 2.0 * rng.standard_normal((points, 5))
            clouds.append((xyz, feat))
        a = 0.004 * (1 + b % 3)
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        t = np.array([0.004, -0.003, 0.002]) * (1 + b % 4)
        xm = clouds[1][0] @ R.T + t
        out.append((clouds[0][0].astype(np.float32), clouds[0][1].astype(np.float32), xm.astype(np.float32),
                    clouds[1][1].astype(np.float32)))
    return out


def _contexts(pkg, mode, pairs, options=()):
    import torch
    capi = pkg.capi
    ctxs, streams = [], []
    for b, pr in enumerate(pairs):
        s = torch.cuda.Stream()
        p = capi.default_params(mode)
        p.max_iter = MAX_ITERS[b % len(MAX_ITERS)]
        c = capi.Context(params=p, device=0, stream=s.cuda_stream, graph_capture=True)
        for key, value in options:
            c.set_option(key, value)
        c.set_fixed(pr[0], pr[1])
        c.set_moving(pr[2], pr[3])
        ctxs.append(c); streams.append(s)
    return ctxs, streams


def _align_many(capi, ctxs, on, reps=2):
    """(two calls each: the second re-uses the engines' captured batches and tables)"""
    for c in ctxs:
        c.set_option("tiles_from_record", on)
    for _ in range(reps):
        states = [capi.init_state(c.params) for c in ctxs]
        its = capi.align_many(ctxs, states)
    stats = [c.list_stats() + (int(c.get_option("tile_rebuilds")),) for c in ctxs]
    return list(its), [bytes(s) for s in states], stats


def _lone(capi, name, ctxs):
    """Every pair of the set registered on its own: computed once per set, shared by the tests that need it."""
    if name not in _LONE:
        res = []
        for c in ctxs:
            st = capi.init_state(c.params)
            n, _ = c.align(st, trace_cap=0)
            res.append((n, bytes(st)))
        _LONE[name] = res
    return _LONE[name]


def _sums(stats):
    return tuple(sum(s[q] for s in stats) for q in range(4))


def _compare(pkg, name, mode, pairs, options=()):
    capi = pkg.capi
    ctxs, streams = _contexts(pkg, mode, pairs, options)
    its_on, st_on, stats_on = _align_many(capi, ctxs, 1)
    its_off, st_off, stats_off = _align_many(capi, ctxs, 0)
    print("%s: builds / narrowings / re-expansions / rebuilds on %s, off %s" % (name, _sums(stats_on), _sums(stats_off)))
    lone = _lone(capi, name, ctxs)
    grows = sum(int(c.get_option("list_grows")) for c in ctxs)
    for c in ctxs:
        c.close()
    assert its_on == its_off
    for b in range(len(pairs)):
        assert st_on[b] == st_off[b], b
        assert its_on[b] == lone[b][0], (b, its_on[b], lone[b][0])
        assert st_on[b] == lone[b][1], b
    assert all(s[3] == 0 for s in stats_off)   # (no rebuilds with the option off)
    return stats_on, stats_off, grows


def test_24_cvo_pairs_mixed_lengths_rebuilt_equal_kept(pkg):
    """(a) 24 x 3 000 points, cvo, max_iter 25 / 60 / 200 mixed: 12 registrations per engine in launches of 16 slots and 128 blocks
    each, then 8 slots and 256 blocks when the short ones have left.  With the option on every drop narrows -- fewer all-pairs
    builds, at least as many narrowings --, lists are rebuilt, and the re-expansions behind them still run."""
    stats_on, stats_off, _ = _compare(pkg, "cvo_24x3k", pkg.capi.MODE_CVO, _surface_pairs(pkg, 24, 3000, False))
    on, off = _sums(stats_on), _sums(stats_off)
    assert on[0] < off[0]
    assert on[1] >= off[1]
    assert on[3] > 0 and on[2] > 0


def test_24_acvo_pairs_mixed_lengths_rebuilt_equal_kept(pkg):
    """(b) the same with acvo: equality."""
    _compare(pkg, "acvo_24x3k", pkg.capi.MODE_ACVO, _surface_pairs(pkg, 24, 3000, True))


def test_16_pairs_of_three_tight_clusters(pkg):
    """(c) 16 pairs of 600 points in three tight clusters, carried by the engines (`small_calls_alone` = 0): launches of 8 slots and
    256 blocks, then 4 and 512 -- several recording blocks per sub-list.  Full 64-bit entries beside single-bit ones, slices that
    end in the middle of an entry."""
    _compare(pkg, "clusters_16x600", pkg.capi.MODE_CVO, _cluster_pairs(16, 600), options=(("small_calls_alone", 0),))


def test_lists_that_begin_with_one_entry_per_sub_list(pkg):
    """(d) `list_init` = 1 on (a)'s set: every list begins far too small and overflows; the loops park, the host grows the lists and
    the registrations resume with an all-pairs build.  A rebuilt list has fewer entries than the build it descends from, so it fits
    once that build did: the test switch `tiles_from_record_cap` = 1 makes every rebuild take its sub-lists for one entry long, which
    sends it down the same road -- the list is void, the loop parks, the list grows, an all-pairs build follows.  That is seen in the
    SECOND call, whose lists are large enough for everything else: they grow again, and no rebuild succeeds.  States still equal
    those of the pairs on their own."""
    capi = pkg.capi
    pairs = _surface_pairs(pkg, 24, 3000, False)
    if "cvo_24x3k" not in _LONE:   # (run on its own: the reference comes from contexts with lists of the usual size)
        ctxs, streams = _contexts(pkg, capi.MODE_CVO, pairs)
        _lone(capi, "cvo_24x3k", ctxs)
        for c in ctxs:
            c.close()
    lone = _LONE["cvo_24x3k"]
    ctxs, streams = _contexts(pkg, capi.MODE_CVO, pairs, options=(("list_init", 1), ("tiles_from_record_cap", 1)))
    grows, runs = [], []
    for on in (1, 1, 0):
        runs.append(_align_many(capi, ctxs, on, reps=1))
        grows.append(sum(int(c.get_option("list_grows")) for c in ctxs))
    for c in ctxs:
        c.close()
    print("list_init 1, rebuilds capped at one entry: lists grown after the calls on / on / off %s; builds / narrowings / re-expansions / "
          "rebuilds %s %s %s" % (grows, _sums(runs[0][2]), _sums(runs[1][2]), _sums(runs[2][2])))
    for its, states, _ in runs:
        for b in range(len(pairs)):
            assert its[b] == lone[b][0], (b, its[b], lone[b][0])
            assert states[b] == lone[b][1], b
    assert grows[0] > 0           # the first lists overflowed
    assert grows[1] > grows[0]    # ... and the second call, the same road over lists the first one sized, parks at its rebuilds alone: the fallback ran
    assert _sums(runs[1][2])[3] == 0   # no rebuild succeeded (the same set rebuilds lists in test (a))
