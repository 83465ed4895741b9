"""-m gpu: cvo_hip_pose_matches (include/cvo_hip.h) against the numpy restatement of tests/pose_matches_ref.py on the
oracle's member sets, against cvo_hip_pose_score / cvo_hip_pose_hessian, and for what it must leave alone.

What is asserted, and why it may be.  The member set and every float32 weight are the oracle's exactly (the project's
arithmetic contract), so count, best and best_w EQUAL the restatement.  A support is accumulated on the device
in 64-bit fixed point in which every weight is an exact integer (summary.exact says so; cvo_matches.hip) and rounded
once to float64: it is the correctly rounded sum of the point's weights, which is what math.fsum of those weights
gives -- so support EQUALS math.fsum per point, in every mode, and lies within 1e-10 relative of the restatement's plain
float64 sums (sums of at most 2^19 positive terms differ between any two orders by less than 2^19 2^-53 ~ 6e-11)."""
import ctypes as C
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_matches_ref as ref  # noqa: E402
from pose_cases import case as _case, ctx as _ctx, pose as _pose, stream as _stream, trace_bits as _trace_bits  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
T0 = np.array([0.02, -0.01, 0.015], np.float32)
NAMES = ("support", "count", "best", "best_w")


def _fsum_per_point(own, val, n):
    """The correctly rounded sum of the float32 weights of every point's members."""
    own = np.asarray(own)
    order = np.argsort(own, kind="stable")
    cuts = np.searchsorted(own[order], np.arange(n + 1))
    v = val.astype(np.float64)[order].tolist()
    return np.array([math.fsum(v[cuts[k]:cuts[k + 1]]) for k in range(n)])


def _bytes(m):
    """The summary of a PoseMatches and every array of either side as bytes."""
    return tuple(m[:8]) + tuple(None if s is None else tuple(a.tobytes() for a in s) for s in (m.fixed, m.moving))


def _check_against(m, want, tag=""):
    """A PoseMatches against the restatement's dict (see the module docstring)."""
    rows, cols, val = want["members"]
    assert m.exact, tag
    assert m.nnz == len(rows), (tag, m.nnz, len(rows))
    for side, own in (("fixed", rows), ("moving", cols)):
        got, w = getattr(m, side), want[side]
        n = len(w[0])
        for k in (1, 2, 3):
            bad = np.flatnonzero(got[k] != w[k])
            print("%s %s %s: %d of %d differ" % (tag, side, NAMES[k], len(bad), n))
            assert len(bad) == 0, (tag, side, NAMES[k], bad[:5], got[k][bad[:5]], w[k][bad[:5]])
        exact = _fsum_per_point(own, val, n)
        rel = np.abs(got.support - w[0]) / np.maximum(w[0], 1e-300)
        print("%s %s support: %d differ from fsum; max relative distance from the float64 sums %.3g"
              % (tag, side, int((got.support != exact).sum()), float(rel.max())))
        assert np.array_equal(got.support, exact), (tag, side)
        assert np.all(np.abs(got.support - w[0]) <= 1e-10 * w[0]), (tag, side)
        assert got.support.dtype == np.float64 and got.count.dtype == np.int32 and got.best.dtype == np.int32 \
            and got.best_w.dtype == np.float32


def _check_summary(m):
    """The arrays against the summary."""
    for side, matched in ((m.fixed, m.fixed_matched), (m.moving, m.moving_matched)):
        assert int(side.count.astype(np.int64).sum()) == m.nnz
        assert int((side.count > 0).sum()) == matched
        tot = math.fsum(side.support.tolist())
        assert abs(tot - m.inner) <= 1e-11 * m.inner, (tot, m.inner)


# ---- 1, 2: oracle parity and consistency with the other calls
@pytest.mark.parametrize("name", ["cvo_3000", "cvo_10000", "desk", "acvo_10000", "matlab_3000"])
def test_matches_restatement_on_oracle_members(pkg, po, desk, name):
    mode, omode, (xf, ff, xm, fm), ell = _case(pkg, desk, name)
    R, T = _pose()
    c = _ctx(pkg, pkg.capi.default_params(mode), xf, ff, xm, fm)
    m = c.pose_matches(R, T, ell)
    s = c.pose_score(R, T, ell)
    h = c.pose_hessian(R, T, ell)
    c.close()
    want = ref.matches(po, omode, ell, xf, ff, xm, fm, R, T)
    assert len(want["members"][0]) > 1000
    _check_against(m, want, name)
    # the summary is pose_score's and the Hessian's, bit for bit
    assert (m.inner, m.nnz, m.fixed_matched, m.moving_matched, m.n_fixed, m.n_moving, m.ell) == \
        (s.inner, s.nnz, s.fixed_matched, s.moving_matched, s.n_fixed, s.n_moving, s.ell)
    assert m.inner == h.f and m.nnz == h.nnz
    assert m.n_fixed == len(xf) and m.n_moving == len(xm) and m.ell == np.float32(ell)
    _check_summary(m)


def test_issue_pose_on_desk(pkg, po, desk):
    """fr1/desk at T = (0.02, -0.01, 0.015), R = I, ell = 0.1: the figures of the CPU oracle."""
    mode, omode, (xf, ff, xm, fm), ell = _case(pkg, desk, "desk")
    c = _ctx(pkg, pkg.capi.default_params(mode), xf, ff, xm, fm)
    m = c.pose_matches(I3, T0, ell)
    c.close()
    assert (m.nnz, m.fixed_matched, m.moving_matched, m.n_fixed, m.n_moving) == (3487424, 15782, 16693, 15849, 17067)
    assert (int(m.fixed.count.max()), int(m.moving.count.max())) == (1200, 1221)
    _check_against(m, ref.matches(po, omode, ell, xf, ff, xm, fm, I3, T0), "desk at R = I")
    _check_summary(m)


# ---- 3: the tie rule and the caller's order
def test_tie_goes_to_the_smallest_index(pkg, po):
    """A cloud against itself with point 100 handed over a second time as point n: the members (100, 100) and (100, n)
    tie at the largest weight there is (d2 = 0, equal features), and so do (n, 100) and (n, n)."""
    x, f, _, _ = pkg.data.synthetic_pair(3000, 3000, seed=19)
    x, f = np.vstack([x, x[100:101]]), np.vstack([f, f[100:101]])
    n = len(x) - 1
    c = _ctx(pkg, pkg.capi.default_params(pkg.capi.MODE_CVO), x, f, x, f)
    m = c.pose_matches(I3, Z3, 0.1)
    c.close()
    want = ref.matches(po, 0, 0.1, x, f, x, f, I3, Z3)
    _check_against(m, want, "duplicate")
    for side in (m.fixed, m.moving):
        assert side.best[100] == 100 and side.best[n] == 100
        assert side.best_w[100] == side.best_w[n] and side.count[100] == side.count[n] and side.support[100] == side.support[n]
        others = np.flatnonzero(side.count > 0)
        others = others[(others != 100) & (others != n)]
        assert np.array_equal(side.best[others], others)
    assert _bytes(m)[8] == _bytes(m)[9]   # (A is symmetric: equal arrays on both sides)


def test_shuffled_clouds_give_shuffled_arrays(pkg):
    capi = pkg.capi
    xf, ff, xm, fm = pkg.data.synthetic_pair(6000, 5500, seed=37)
    R, T = _pose()
    rng = np.random.default_rng(3)
    pf, pm = rng.permutation(len(xf)), rng.permutation(len(xm))
    inv_f, inv_m = np.argsort(pf), np.argsort(pm)
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    a = c.pose_matches(R, T, 0.1)
    c.set_fixed(xf[pf], ff[pf])
    c.set_moving(xm[pm], fm[pm])
    b = c.pose_matches(R, T, 0.1)
    c.close()
    assert a[:8] == b[:8] and a.nnz > 1000
    for sa, sb, perm, inv_other in ((a.fixed, b.fixed, pf, inv_m), (a.moving, b.moving, pm, inv_f)):
        for k in (0, 1, 3):
            assert np.array_equal(sb[k], sa[k][perm]), NAMES[k]
        best = sa.best[perm]
        assert np.array_equal(sb.best, np.where(best >= 0, inv_other[np.maximum(best, 0)], -1))


# ---- 4: every kept format, a list that grows, every hand-over path
def test_kept_format_0_and_both_forms_of_the_pass(pkg, po):
    xf, ff, xm, fm = pkg.data.synthetic_pair(10000, 10000, seed=13)
    R, T = _pose()
    c = _ctx(pkg, pkg.capi.default_params(pkg.capi.MODE_CVO), xf, ff, xm, fm)
    packed = c.pose_matches(R, T, 0.1)
    c.set_option("matches_combine", 0)
    plain = c.pose_matches(R, T, 0.1)
    c.set_option("kept_pack", 0)
    wide_plain = c.pose_matches(R, T, 0.1)
    c.set_option("matches_combine", 1)
    wide = c.pose_matches(R, T, 0.1)
    c.close()
    _check_against(wide, ref.matches(po, 0, 0.1, xf, ff, xm, fm, R, T), "16-byte entries")
    assert _bytes(packed) == _bytes(plain) == _bytes(wide_plain) == _bytes(wide)


def test_kept_format_2(pkg, po):
    """Clouds above 65 536 rows: 8-byte entries with the weight's exponent packed (ProcessArgs::kept_packed == 2)."""
    xf, ff, xm, fm = pkg.data.synthetic_pair(70000, 70000, seed=17)
    R, T = _pose()
    c = _ctx(pkg, pkg.capi.default_params(pkg.capi.MODE_CVO), xf, ff, xm, fm)
    m = c.pose_matches(R, T, 0.03)
    c.set_option("matches_combine", 0)
    plain = c.pose_matches(R, T, 0.03)
    c.close()
    want = ref.matches(po, 0, 0.03, xf, ff, xm, fm, R, T)
    assert len(want["members"][0]) > 10000
    _check_against(m, want, "exponent-packed entries")
    _check_summary(m)
    assert _bytes(m) == _bytes(plain)


def test_lists_that_overflow_are_grown(pkg):
    capi = pkg.capi
    xf, ff, xm, fm = pkg.data.synthetic_pair(10000, 10000, seed=13)
    R, T = _pose()
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    want = c.pose_matches(R, T, 0.1)
    c.close()
    c = capi.Context(params=capi.default_params(capi.MODE_CVO), device=0, stream=_stream())
    c.set_option("list_init", 1)   # the minimum capacity of every list: the first pass overflows them
    c.set_fixed(xf, ff)
    c.set_moving(xm, fm)
    got = c.pose_matches(R, T, 0.1)
    again = c.pose_matches(R, T, 0.1)
    c.close()
    assert want.nnz > 100000
    assert _bytes(got) == _bytes(want) == _bytes(again)


def test_every_hand_over_path_keeps_the_callers_index(pkg):
    """Host arrays (the one-launch and the multi-launch preparation), device arrays in both feature layouts, a batched
    hand-over, and a cloud that cvo_hip_swap_moving_to_fixed moved: equal arrays."""
    import torch
    capi = pkg.capi
    p = capi.default_params(capi.MODE_CVO)
    R, T = _pose()
    for n in (3000, 40000):   # (a cloud the one-launch preparation takes, and one it does not)
        xf, ff, xm, fm = pkg.data.synthetic_pair(n, n - 123, seed=61)
        ell = 0.1 if n == 3000 else 0.04
        c = _ctx(pkg, p, xf, ff, xm, fm)
        want = _bytes(c.pose_matches(R, T, ell))
        c.close()
        assert want[1] > 1000
        # the multi-launch preparation
        c = capi.Context(params=p, device=0, stream=_stream())
        c.set_option("one_launch_hand_over", 0)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        assert _bytes(c.pose_matches(R, T, ell)) == want
        c.close()
        # device arrays, row- and column-major features
        for lay in (capi.FEAT_ROWMAJOR, capi.FEAT_COLMAJOR):
            host = [xf, ff if lay == capi.FEAT_ROWMAJOR else np.ascontiguousarray(ff.T),
                    xm, fm if lay == capi.FEAT_ROWMAJOR else np.ascontiguousarray(fm.T)]
            t = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in host]
            c = capi.Context(params=p, device=0, stream=_stream())
            c.set_fixed_device(t[0].data_ptr(), t[1].data_ptr(), len(xf), lay)
            c.set_moving_device(t[2].data_ptr(), t[3].data_ptr(), len(xm), lay)
            assert _bytes(c.pose_matches(R, T, ell)) == want, lay
            c.close()
        # a batched hand-over
        cs = [capi.Context(params=p, device=0, stream=_stream()) for _ in range(2)]
        capi.set_pcd_many(cs, [(xf, ff)] * 2, [(xm, fm)] * 2)
        for c in cs:
            assert _bytes(c.pose_matches(R, T, ell)) == want
            c.close()
        # the fixed cloud came as a moving one
        c = capi.Context(params=p, device=0, stream=_stream())
        c.set_fixed(xm, fm)
        c.set_moving(xf, ff)
        c.swap_moving_to_fixed()
        c.set_moving(xm, fm)
        assert _bytes(c.pose_matches(R, T, ell)) == want
        c.close()


def test_front_end_cloud(pkg):
    """The front end's cloud handed over on the device against the same cloud from host arrays."""
    capi = pkg.capi
    bgr, dep = pkg.data.synthetic_rgbd_frame(seed=5, texture=1.0)
    gen = pkg.frontend.PcdGenerator(640, 480)
    xyz, feat = gen.create_pointcloud(bgr, dep, dataset_seq=1, feature_type=pkg.frontend.FEATURES_RGB)
    p = capi.default_params(capi.MODE_CVO)
    T = np.array([0.01, -0.005, 0.01], np.float32)
    c = _ctx(pkg, p, xyz, feat, xyz, feat)
    want = c.pose_matches(I3, T, 0.1)
    c.close()
    assert want.nnz > 1000 and want.n_fixed == len(xyz)
    c = capi.Context(params=p, device=0, stream=_stream())
    gen.set_device_output(True)
    for put in (c.set_fixed_device, c.set_moving_device):
        gen.submit(bgr, dep, 1, pkg.frontend.FEATURES_RGB)
        d_xyz, d_feat, npts = gen.collect_device()
        assert npts == len(xyz)
        put(d_xyz, d_feat, npts)
    got = c.pose_matches(I3, T, 0.1)
    c.close()
    gen.close()
    assert _bytes(got) == _bytes(want)


# ---- 5, 6: determinism; one side only
def test_repeated_calls_are_byte_identical(pkg, desk):
    capi = pkg.capi
    mode, _, (xf, ff, xm, fm), ell = _case(pkg, desk, "desk")
    x2, f2, _, _ = pkg.data.synthetic_pair(4000, 4000, seed=53)
    R, T = _pose()
    c = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
    first = _bytes(c.pose_matches(R, T, ell))
    assert first == _bytes(c.pose_matches(R, T, ell)) == _bytes(c.pose_matches(R, T, ell))
    c.set_moving(x2, f2)
    other = c.pose_matches(R, T, ell)
    c.set_moving(xm, fm)
    back = _bytes(c.pose_matches(R, T, ell))
    c.close()
    assert other.n_moving == 4000 and len(other.moving.count) == 4000
    assert back == first


def test_one_side_only_and_no_arrays(pkg):
    capi = pkg.capi
    xf, ff, xm, fm = pkg.data.synthetic_pair(5000, 4500, seed=47)
    R, T = _pose()
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    both = c.pose_matches(R, T, 0.1)
    only_f = c.pose_matches(R, T, 0.1, moving=False)
    only_m = c.pose_matches(R, T, 0.1, fixed=False)
    none = c.pose_matches(R, T, 0.1, fixed=False, moving=False)
    # a single array through the C ABI: the others stay null
    cnt = np.full(len(xm), 7, np.int32)
    side = capi.PointMatchesC(None, cnt.ctypes.data_as(C.POINTER(C.c_int32)), None, None)
    out = capi.PoseMatchesC()
    Rc, Tc = np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(T)
    rc = capi.lib().cvo_hip_pose_matches(c._ctx, capi.fptr(Rc), capi.fptr(Tc), np.float32(0.1), None, C.byref(side), C.byref(out))
    c.close()
    assert rc == 0 and np.array_equal(cnt, both.moving.count)
    assert both[:8] == only_f[:8] == only_m[:8] == none[:8] and both.nnz == out.nnz and both.inner == out.inner
    assert only_f.moving is None and only_m.fixed is None and none.fixed is None and none.moving is None
    assert _bytes(both)[8] == _bytes(only_f)[8] and _bytes(both)[9] == _bytes(only_m)[9]


# ---- 7: no side effects
@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_no_side_effects_on_align(pkg, mode_name):
    capi = pkg.capi
    mode = capi.MODE_ACVO if mode_name == "acvo" else capi.MODE_CVO
    xf, ff, xm, fm = pkg.data.synthetic_pair(3000, 3000, seed=31, acvo=mode_name == "acvo")
    R, T = _pose()
    runs = []
    for with_m in (False, True):
        c = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
        if with_m:
            c.pose_matches(R, T, 0.1)
        st = capi.init_state(c.params)
        n, tr = c.align(st, trace_cap=2000)
        runs.append((n, _trace_bits(tr), bytes(st)))
        if with_m:   # ... and after an align the answer at the pose is what a fresh context gives
            after = _bytes(c.pose_matches(R, T, 0.1))
        c.close()
    assert runs[0] == runs[1]
    c = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
    assert _bytes(c.pose_matches(R, T, 0.1)) == after
    c.close()


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_run_sequence_with_matches(pkg, desk, mode_name):
    Reg = pkg.Acvo if mode_name == "acvo" else pkg.Cvo
    feats = pkg.data.acvo_features if mode_name == "acvo" else pkg.data.cvo_features
    frames = [(str(k), desk["xyz%d" % k], feats(desk["rgb%d" % k])) for k in range(5)]
    out = []
    for matches in (False, True):
        reg = Reg(device=0, stream=_stream())
        iters = reg.run_sequence(iter(frames), matches=matches)
        out.append((iters, reg.accum_transform.tobytes(), reg.transform.tobytes()))
        got, last = list(reg.matches_list), reg.matches
        ell_init = np.float32(reg.params.ell_init)
        reg.close()
        if not matches:
            assert got == [] and last is None
    assert out[0] == out[1]
    assert len(got) == 4 and got[-1] is last
    for k, m in enumerate(got):
        assert m.ell == ell_init and m.nnz > 0 and m.exact
        assert len(m.fixed.count) == len(frames[k][1]) and len(m.moving.count) == len(frames[k + 1][1])
        assert m.fixed_matched > len(frames[k][1]) // 2
        _check_summary(m)


# ---- 8: refusals and the empty set
def test_refusals_and_empty_set(pkg):
    capi = pkg.capi
    p = capi.default_params(capi.MODE_CVO)
    xf, ff, xm, fm = pkg.data.synthetic_pair(2000, 2100, seed=41)
    R, T = _pose()
    c = _ctx(pkg, p, xf, ff, xm, fm)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(capi.CvoHipError):
            c.pose_matches(R, T, bad)
    out = capi.PoseMatchesC()
    Rc, Tc = np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(T)
    L = capi.lib()
    assert L.cvo_hip_pose_matches(c._ctx, None, capi.fptr(Tc), np.float32(0.1), None, None, C.byref(out)) == -1
    assert L.cvo_hip_pose_matches(c._ctx, capi.fptr(Rc), None, np.float32(0.1), None, None, C.byref(out)) == -1
    assert L.cvo_hip_pose_matches(c._ctx, capi.fptr(Rc), capi.fptr(Tc), np.float32(0.1), None, None, None) == -1
    # far apart: no member at all -- zeros, -1 and OK
    c.set_moving(xm + np.float32(100.0), fm)
    m = c.pose_matches(R, T, 0.1)
    assert (m.nnz, m.inner, m.fixed_matched, m.moving_matched, m.n_fixed, m.n_moving) == (0, 0.0, 0, 0, 2000, 2100)
    for side in (m.fixed, m.moving):
        assert not side.support.any() and not side.count.any() and not side.best_w.any() and np.all(side.best == -1)
    # a shard over the whole clouds is the whole registration; a narrower one is refused
    c.set_moving(xm, fm)
    whole = c.pose_matches(R, T, 0.1)
    c.set_shard(0, len(xf), 0, len(xm))
    assert _bytes(c.pose_matches(R, T, 0.1))[1:] == _bytes(whole)[1:]
    c.set_shard(0, len(xf) // 2, 0, len(xm))
    with pytest.raises(capi.CvoHipError, match="shard"):
        c.pose_matches(R, T, 0.1)
    c.close()
    # a cloud missing
    c = capi.Context(params=p, device=0, stream=_stream())
    c.set_fixed(xf, ff)
    with pytest.raises(capi.CvoHipError):
        c.pose_matches(R, T, 0.1)
    c.close()
    # an all-reduce hook, mailboxes attached
    c = _ctx(pkg, p, xf, ff, xm, fm)
    c.set_allreduce(lambda buf, count, stream: None)
    with pytest.raises(capi.CvoHipError, match="all-reduce"):
        c.pose_matches(R, T, 0.1)
    c.close()
    c = _ctx(pkg, p, xf, ff, xm, fm)
    c.mailbox_create(0, 1)
    with pytest.raises(capi.CvoHipError, match="mailboxes"):
        c.pose_matches(R, T, 0.1)
    c.close()


# ---- 9: the C++ mirror
def _fnv1a(b):
    h = 0xcbf29ce484222325
    for v in b:
        h = ((h ^ v) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_cpp_mirror_matches_python(pkg, tmp_path):
    lib = os.path.join(ROOT, "cvo-rgbd_amd", "csrc")
    exe = str(tmp_path / "cvo_matches_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "cvo_matches_demo.cpp"), "-L", lib, "-lcvo_hip",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    xf, ff, xm, fm = pkg.data.synthetic_pair(4000, 3800, seed=67)
    R, T = _pose()
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", 2))
        for x, f in ((xf, ff), (xm, fm)):
            fh.write(struct.pack("<i", len(x)))
            fh.write(np.ascontiguousarray(x, np.float32).tobytes())
            fh.write(np.ascontiguousarray(f, np.float32).tobytes())
        fh.write(R.astype(np.float32).tobytes() + T.astype(np.float32).tobytes() + np.float32(0.1).tobytes())
    lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    tok = dict((ln.split()[0], ln.split()[1]) for ln in lines)
    c = _ctx(pkg, pkg.capi.default_params(pkg.capi.MODE_CVO), xf, ff, xm, fm)
    m = c.pose_matches(R, T, 0.1)
    c.close()
    assert m.nnz > 1000
    for k in ("nnz", "n_fixed", "n_moving", "fixed_matched", "moving_matched"):
        assert int(tok[k]) == getattr(m, k), k
    assert int(tok["exact"]) == int(m.exact)
    assert float.fromhex(tok["inner"]) == m.inner and float.fromhex(tok["ell"]) == m.ell
    for side in ("fixed", "moving"):
        for k, name in enumerate(NAMES):
            assert int(tok["%s_%s" % (side, name)], 16) == _fnv1a(getattr(m, side)[k].tobytes()), (side, name)
