"""-m gpu: cvo_hip_pose_score / cvo_hip_pose_score_many (include/cvo_hip.h) against the float64 restatement of
tests/pose_score_ref.py on the oracle's member sets, against cvo_hip_pose_hessian, and for what they must leave alone.

Tolerances.  The member sets and every float32 weight are the oracle's exactly (counts equal, sums of a to 1e-11); a d2
is the kernels' fma form against float64 squares of the float32 differences (mean_d2 to 1e-6)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_score_ref as ref  # noqa: E402
from pose_cases import case as _case, ctx as _ctx, pose as _pose, stream as _stream, trace_bits as _trace_bits  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


def _check(got, want):
    for k in ("nnz", "nnz_fixed", "nnz_moving", "fixed_matched", "moving_matched"):
        assert getattr(got, k) == want[k], (k, getattr(got, k), want[k])
    for k in ("inner", "self_fixed", "self_moving"):
        assert abs(getattr(got, k) - want[k]) <= 1e-11 * want[k], (k, getattr(got, k), want[k])
    assert abs(got.mean_d2 - want["mean_d2"]) <= 1e-6 * want["mean_d2"]
    assert abs(got.cos_angle - want["cos_angle"]) <= 1e-10


@pytest.mark.parametrize("name", ["cvo_3000", "cvo_10000", "desk", "acvo_10000", "matlab_3000"])
def test_matches_restatement_on_oracle_members(pkg, po, desk, name):
    mode, omode, (xf, ff, xm, fm), ell = _case(pkg, desk, name)
    R, T = _pose()
    c = _ctx(pkg, pkg.capi.default_params(mode), xf, ff, xm, fm)
    got = c.pose_score(R, T, ell)
    h = c.pose_hessian(R, T, ell)
    c.close()
    want = ref.score(po, omode, ell, xf, ff, xm, fm, R, T)
    assert want["nnz"] > 1000 and 0.0 < want["cos_angle"] < 1.0
    _check(got, want)
    assert got.n_fixed == len(xf) and got.n_moving == len(xm) and got.ell == np.float32(ell)
    assert abs(got.rms - np.sqrt(want["mean_d2"])) <= 1e-6 * np.sqrt(want["mean_d2"])
    # the cross term is the Hessian's f, bit for bit
    assert got.inner == h.f and got.nnz == h.nnz


def test_one_cloud_on_both_sides(pkg, po):
    """A cloud against itself at the identity: the three sums are one sum.  3001 points: the device arrays carry 255
    padding rows (NaN features), which must not become members of the self sets."""
    capi = pkg.capi
    x, f, _, _ = pkg.data.synthetic_pair(3001, 3001, seed=43)
    for mode in (capi.MODE_CVO, capi.MODE_ACVO):
        c = _ctx(pkg, capi.default_params(mode), x, f, x, f)
        s = c.pose_score(I3, Z3, 0.1)
        c.close()
        assert s.nnz == s.nnz_fixed == s.nnz_moving
        for v in (s.self_fixed, s.self_moving):
            assert abs(s.inner - v) <= 1e-12 * v
        assert abs(s.cos_angle - 1.0) <= 1e-12
        assert s.fixed_matched == s.moving_matched == len(x)
        want = ref.score(po, 0 if mode == capi.MODE_CVO else 1, 0.1, x, f, x, f, I3, Z3)
        assert s.nnz_fixed == want["nnz_fixed"]


def test_repeated_and_cached_calls_are_bit_identical(pkg):
    capi = pkg.capi
    xf, ff, xm, fm = pkg.data.synthetic_pair(10000, 10000, seed=29)
    R, T = _pose()
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    cold = bytes(c.pose_score_raw(R, T, 0.1))   # both norms computed
    warm = bytes(c.pose_score_raw(R, T, 0.1))   # both from the clouds' caches
    again = bytes(c.pose_score_raw(R, T, 0.1))
    other = c.pose_score(R, T, 0.12)            # another ell: computed again ...
    back = bytes(c.pose_score_raw(R, T, 0.1))   # ... and back
    c.close()
    assert cold == warm == again == back
    assert other.self_fixed != capi.PoseScoreC.from_buffer_copy(cold).self_fixed


def _fresh_self(pkg, params, x, f, other):
    """self_fixed of a fresh context with x as its fixed cloud."""
    c = _ctx(pkg, params, x, f, *other)
    s = c.pose_score(I3, Z3, 0.1)
    c.close()
    return s


def test_cache_follows_the_clouds(pkg):
    capi = pkg.capi
    p = capi.default_params(capi.MODE_CVO)
    x0, f0, x1, f1 = pkg.data.synthetic_pair(5000, 5000, seed=47)
    x2, f2, x3, f3 = pkg.data.synthetic_pair(4000, 4000, seed=53)
    c = _ctx(pkg, p, x0, f0, x1, f1)
    s01 = c.pose_score(I3, Z3, 0.1)
    c.swap_moving_to_fixed()
    c.set_moving(x2, f2)
    s12 = c.pose_score(I3, Z3, 0.1)
    # carried along: cloud 1's norm as a moving cloud is its norm as a fixed one, and a fresh context's
    assert s12.self_fixed == s01.self_moving and s12.nnz_fixed == s01.nnz_moving
    fresh1 = _fresh_self(pkg, p, x1, f1, (x2, f2))
    assert s12.self_fixed == fresh1.self_fixed and s12.nnz_fixed == fresh1.nnz_fixed
    # a new fixed cloud: recomputed, not the stale one
    c.set_fixed(x3, f3)
    s32 = c.pose_score(I3, Z3, 0.1)
    fresh3 = _fresh_self(pkg, p, x3, f3, (x2, f2))
    assert s32.self_fixed == fresh3.self_fixed != s12.self_fixed
    assert s32.self_moving == s12.self_moving
    # new parameters: recomputed
    q = capi.default_params(capi.MODE_CVO)
    q.sp_thres = p.sp_thres * 4.0
    c.set_params(q)
    sq = c.pose_score(I3, Z3, 0.1)
    c.close()
    assert sq.nnz_fixed < s32.nnz_fixed and sq.nnz_moving < s32.nnz_moving
    assert _fresh_self(pkg, q, x3, f3, (x2, f2)).self_fixed == sq.self_fixed
    assert _fresh_self(pkg, q, x2, f2, (x3, f3)).self_fixed == sq.self_moving


def _batch(pkg, k0=0):
    """Clouds, params, poses and ells of 18 registrations, cvo and acvo mixed."""
    capi = pkg.capi
    items = []
    for k in range(18):
        acvo = k % 3 == 2
        n = (2000, 3500, 6000)[k % 3]
        clouds = pkg.data.synthetic_pair(n, n + 37 * k, seed=100 + k + k0, acvo=acvo)
        ax = np.array([0.1 * k, 1.0, -0.3])
        ax /= np.linalg.norm(ax)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        th = 0.005 * (k % 5)
        R = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).astype(np.float32)
        T = np.array([0.002 * k, -0.01, 0.003], np.float32)
        items.append((capi.default_params(capi.MODE_ACVO if acvo else capi.MODE_CVO), clouds, R, T,
                      0.1 if k % 2 else 0.08))
    return items


def test_many_equals_lone_calls(pkg):
    capi = pkg.capi
    items = _batch(pkg)
    Rs, Ts, ells = [it[2] for it in items], [it[3] for it in items], [it[4] for it in items]
    lone = []
    for p, cl, R, T, ell in items:
        c = _ctx(pkg, p, *cl)
        lone.append(bytes(c.pose_score_raw(R, T, ell)))
        c.close()
    ctxs = [_ctx(pkg, p, *cl) for p, cl, _, _, _ in items]
    try:
        got = [bytes(s) for s in capi.pose_score_many_raw(ctxs, Rs, Ts, ells)]   # cold caches
        assert got == lone
        warm = [bytes(s) for s in capi.pose_score_many_raw(ctxs, Rs, Ts, ells)]  # warm caches
        assert warm == lone
        assert [capi.pose_score_from_c(capi.PoseScoreC.from_buffer_copy(b)) for b in lone] == \
            capi.pose_score_many(ctxs, Rs, Ts, ells)
        # after an align_many on the same contexts: the lists have other sizes, the scores are the same
        states = [capi.init_state(c.params) for c in ctxs]
        capi.align_many(ctxs, states)
        after = [bytes(s) for s in capi.pose_score_many_raw(ctxs, Rs, Ts, ells)]
        assert after == lone
    finally:
        for c in ctxs:
            c.close()
    # fresh contexts loaded with the same clouds by one batched hand-over
    ctxs = [capi.Context(params=p, device=0, stream=_stream()) for p, _, _, _, _ in items]
    try:
        capi.set_pcd_many(ctxs, [(cl[0], cl[1]) for _, cl, _, _, _ in items], [(cl[2], cl[3]) for _, cl, _, _, _ in items])
        assert [bytes(s) for s in capi.pose_score_many_raw(ctxs, Rs, Ts, ells)] == lone
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_no_side_effects_on_align(pkg, mode_name):
    capi = pkg.capi
    mode = capi.MODE_ACVO if mode_name == "acvo" else capi.MODE_CVO
    xf, ff, xm, fm = pkg.data.synthetic_pair(3000, 3000, seed=31, acvo=mode_name == "acvo")
    R, T = _pose()
    runs = []
    for with_s in (False, True):
        c = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
        if with_s:
            c.pose_score(R, T, 0.1)
        st = capi.init_state(c.params)
        n, tr = c.align(st, trace_cap=2000)
        runs.append((n, _trace_bits(tr), bytes(st)))
        c.close()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_run_sequence_with_score(pkg, desk, mode_name):
    Reg = pkg.Acvo if mode_name == "acvo" else pkg.Cvo
    feats = pkg.data.acvo_features if mode_name == "acvo" else pkg.data.cvo_features
    frames = [(str(k), desk["xyz%d" % k], feats(desk["rgb%d" % k])) for k in range(5)]
    out = []
    for score in (False, True):
        reg = Reg(device=0, stream=_stream())
        poses = []
        iters = reg.run_sequence(iter(frames), score=score)
        poses.append(reg.accum_transform.tobytes())
        scores = list(reg.scores)
        ell_init = np.float32(reg.params.ell_init)
        reg.close()
        out.append((iters, poses))
    assert out[0] == out[1]
    assert len(scores) == 4
    for k, s in enumerate(scores):
        assert s.ell == ell_init and 0.5 < s.cos_angle < 1.0 and s.nnz > 0
        if k + 1 < len(scores):
            assert s.self_moving == scores[k + 1].self_fixed and s.nnz_moving == scores[k + 1].nnz_fixed


def test_refusals_and_empty_set(pkg):
    capi = pkg.capi
    p = capi.default_params(capi.MODE_CVO)
    xf, ff, xm, fm = pkg.data.synthetic_pair(2000, 2000, seed=41)
    R, T = _pose()
    c = _ctx(pkg, p, xf, ff, xm, fm)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(capi.CvoHipError):
            c.pose_score(R, T, bad)
    # far apart: no member at all -- zeros and OK
    c.set_moving(xm + np.float32(100.0), fm)
    s = c.pose_score(R, T, 0.1)
    assert s.nnz == 0 and s.inner == 0.0 and s.cos_angle == 0.0 and s.mean_d2 == 0.0
    assert s.fixed_matched == 0 and s.moving_matched == 0 and s.self_fixed > 0 and s.self_moving > 0
    # a shard over the whole clouds is the whole registration; a narrower one is refused
    c.set_moving(xm, fm)
    whole = c.pose_score(R, T, 0.1)
    c.set_shard(0, len(xf), 0, len(xm))
    sh = c.pose_score(R, T, 0.1)
    assert (sh.nnz, sh.fixed_matched, sh.moving_matched, sh.self_fixed) == \
        (whole.nnz, whole.fixed_matched, whole.moving_matched, whole.self_fixed)
    assert abs(sh.inner - whole.inner) <= 1e-12 * whole.inner
    c.set_shard(0, len(xf) // 2, 0, len(xm))
    with pytest.raises(capi.CvoHipError, match="shard"):
        c.pose_score(R, T, 0.1)
    c.close()
    # a cloud missing
    c = capi.Context(params=p, device=0, stream=_stream())
    c.set_fixed(xf, ff)
    with pytest.raises(capi.CvoHipError):
        c.pose_score(R, T, 0.1)
    c.close()
    # an all-reduce hook, mailboxes attached
    c = _ctx(pkg, p, xf, ff, xm, fm)
    c.set_allreduce(lambda buf, count, stream: None)
    with pytest.raises(capi.CvoHipError, match="all-reduce"):
        c.pose_score(R, T, 0.1)
    c.close()
    c = _ctx(pkg, p, xf, ff, xm, fm)
    c.mailbox_create(0, 1)
    with pytest.raises(capi.CvoHipError, match="mailboxes"):
        c.pose_score(R, T, 0.1)
    # ... and in a batch: refused before any context is touched
    d = _ctx(pkg, p, xf, ff, xm, fm)
    with pytest.raises(capi.CvoHipError):
        capi.pose_score_many([d, c], [R, R], [T, T], [0.1, 0.1])
    with pytest.raises(capi.CvoHipError):
        capi.pose_score_many([d, d], [R, R], [T, T], [0.1, 0.1])
    with pytest.raises(capi.CvoHipError):
        capi.pose_score_many([d], [R], [T], [float("nan")])
    assert capi.pose_score_many([], [], [], []) == []
    c.close()
    d.close()


def test_cross_device_batch_is_refused(pkg):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible: contexts on two devices need a second one")
    capi = pkg.capi
    xf, ff, xm, fm = pkg.data.synthetic_pair(2000, 2000, seed=59)
    cs = []
    for dev in (0, 1):
        c = capi.Context(params=capi.default_params(capi.MODE_CVO), device=dev)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        cs.append(c)
    with pytest.raises(capi.CvoHipError):
        capi.pose_score_many(cs, [I3, I3], [Z3, Z3], [0.1, 0.1])
    for c in cs:
        c.close()


def test_cpp_mirror_matches_python(pkg, desk, tmp_path):
    lib = os.path.join(ROOT, "cvo-rgbd_amd", "csrc")
    exe = str(tmp_path / "cvo_score_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "cvo_score_demo.cpp"), "-L", lib, "-lcvo_hip",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    frames = [(desk["xyz%d" % k], pkg.data.cvo_features(desk["rgb%d" % k])) for k in range(2)]
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(frames)))
        for x, f in frames:
            fh.write(struct.pack("<i", len(x)))
            fh.write(np.ascontiguousarray(x, np.float32).tobytes())
            fh.write(np.ascontiguousarray(f, np.float32).tobytes())
    lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    reg = pkg.Cvo(device=0)
    reg.set_pcd(*frames[0])
    reg.set_pcd(*frames[1])
    reg.align(hessian=True, score=True)
    s, h, n_iter = reg.score, reg.hessian, reg.num_iterations
    reg.close()
    tok = dict((ln.split()[0], ln.split()[1]) for ln in lines)
    assert int(tok["n_iter"]) == n_iter
    for k in ("nnz", "nnz_fixed", "nnz_moving", "fixed_matched", "moving_matched"):
        assert int(tok[k]) == getattr(s, k), k
    for k in ("inner", "self_fixed", "self_moving", "cos_angle", "mean_d2", "ell"):
        assert float.fromhex(tok[k]) == getattr(s, k), k
    assert float.fromhex(tok["hess_f"]) == h.f
