"""-m gpu: cvo_hip_pose_scan (include/cvo_hip.h) against the float64 restatement of tests/pose_scan_ref.py on the oracle's
member sets, against cvo_hip_pose_score on the same context, for the independence of an entry from the call it is part
of, for the padding rows of the device clouds, for the state it leaves, and end to end on the displaced pairs of
tests/test_pose_scan_cpu.py.

Tolerances.  Member sets and float32 weights are the oracle's and cvo_hip_pose_score's exactly, so counts are equal and
two float64 sums of the same nnz positive terms differ by at most 2 g inner, g = nnz u / (1 - nnz u), u = 2^-53;
mean_d2 against the score is two such sums and a division each (4 g + 4 u), against the restatement the existing
score test's 1e-6 (its d2 is float64 squares of the float32 differences); cosines to 1e-10."""
import ctypes
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_scan_ref as sref  # noqa: E402
from pose_cases import case as _case, ctx as _ctx, pose as _pose, stream as _stream, trace_bits as _trace_bits  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


def _entries(pkg, raw):
    return np.frombuffer(raw, pkg.capi.POSE_SCAN_ENTRY)


@pytest.mark.parametrize("name", ["cvo_3000", "acvo_10000", "matlab_3000", "desk"])
def test_matches_restatement_and_pose_score(pkg, po, desk, name):
    mode, omode, (xf, ff, xm, fm), ell = _case(pkg, desk, name)
    Rs, Ts = sref.accuracy_poses(*_pose())
    assert len(Rs) == 25
    c = _ctx(pkg, pkg.capi.default_params(mode), xf, ff, xm, fm)
    got = c.pose_scan(Rs, Ts, ell)
    scores = [c.pose_score(Rs[k], Ts[k], ell) for k in range(len(Rs))]
    c.close()
    want = sref.scan(po, omode, ell, xf, ff, xm, fm, Rs, Ts)
    print(name, "nnz", got.nnz.tolist(), "best", got.best, want["best"])
    assert want["nnz"][0] > 1000 and want["nnz"][22] == 0 == want["nnz"][23] and int(np.sum(want["nnz"] > 0)) >= 20
    assert got.count == 25 and got.n_fixed == len(xf) and got.n_moving == len(xm) and got.ell == np.float32(ell)
    # the restatement
    assert np.array_equal(got.nnz, want["nnz"])
    assert got.nnz_fixed == want["nnz_fixed"] and got.nnz_moving == want["nnz_moving"]
    for k in range(25):
        g = sref.gamma(int(want["nnz"][k]))
        print(k, int(got.nnz[k]), abs(got.inner[k] - want["inner"][k]), 2 * g * want["inner"][k],
              abs(got.mean_d2[k] - want["mean_d2"][k]), abs(got.cos_angle[k] - want["cos_angle"][k]))
        assert abs(got.inner[k] - want["inner"][k]) <= 2 * g * want["inner"][k], k
        assert abs(got.mean_d2[k] - want["mean_d2"][k]) <= 1e-6 * want["mean_d2"][k], k
        assert abs(got.cos_angle[k] - want["cos_angle"][k]) <= 1e-10, k
    assert got.best == want["best"]
    # cvo_hip_pose_score on the same context
    for k, s in enumerate(scores):
        g = sref.gamma(s.nnz)
        assert got.nnz[k] == s.nnz, k
        assert (got.self_fixed, got.self_moving, got.nnz_fixed, got.nnz_moving) == (s.self_fixed, s.self_moving, s.nnz_fixed, s.nnz_moving)
        assert abs(got.inner[k] - s.inner) <= 2 * g * s.inner, k
        assert abs(got.mean_d2[k] - s.mean_d2) <= (4 * g + 4 * sref.U) * s.mean_d2, k


def _scenario_poses(pkg, po, sc):
    """The scenario's 343-pose grid followed by the 25 accuracy poses around the grid's recorded winner: 368 poses."""
    Rg, Tg = sref.scenario_grid()
    Ra, Ta = sref.accuracy_poses(Rg[sc["winner"]], Tg[sc["winner"]])
    return np.concatenate([Rg, Ra]), np.concatenate([Tg, Ta])


def test_an_entry_does_not_depend_on_the_call(pkg, po):
    capi = pkg.capi
    sc = sref.SCENARIOS[0]
    xf, ff, xm, fm = sref.scenario_clouds(pkg, sc)
    ell = sref.SCENARIO_ELL
    Rs, Ts = _scenario_poses(pkg, po, sc)
    n = len(Rs)
    assert n == 368
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    full, summary = c.pose_scan_raw(Rs, Ts, ell)
    ent = _entries(pkg, full)
    assert len(full) == 32 * n and int(np.sum(ent["nnz"] == 0)) >= sc["empty"] and int(np.sum(ent["nnz"] > 0)) >= 40
    one = lambda k: full[32 * k:32 * k + 32]   # noqa: E731
    # a random permutation
    perm = np.random.Generator(np.random.PCG64(5)).permutation(n)
    raw, _ = c.pose_scan_raw(Rs[perm], Ts[perm], ell)
    for q, k in enumerate(perm):
        assert raw[32 * q:32 * q + 32] == one(k), k
    # alone: five poses with members, five without
    alone = list(np.flatnonzero(ent["nnz"] > 0)[[0, 7, 15, 30, -1]]) + list(np.flatnonzero(ent["nnz"] == 0)[[0, 50, 100, 200, -1]])
    for k in alone:
        raw, s1 = c.pose_scan_raw(Rs[k:k + 1], Ts[k:k + 1], ell)
        assert raw == one(k), k
        assert s1.best == (0 if ent["nnz"][k] > 0 else -1)
    # the list twice in one call
    raw, s2 = c.pose_scan_raw(np.concatenate([Rs, Rs]), np.concatenate([Ts, Ts]), ell)
    assert raw == full + full and s2.best == summary.best
    # after an align() and a score at another ell on the context
    st = capi.init_state(c.params)
    c.align(st)
    c.pose_score(Rs[summary.best], Ts[summary.best], 0.08)
    raw, s3 = c.pose_scan_raw(Rs, Ts, ell)
    assert raw == full and bytes(s3) == bytes(summary)
    # however the call is cut into launches
    for chunk in (1, 7, 0):
        c.set_option("scan_chunk", chunk)
        raw, s4 = c.pose_scan_raw(Rs, Ts, ell)
        assert raw == full and bytes(s4) == bytes(summary), chunk
    c.close()
    # a fresh context
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    raw, s5 = c.pose_scan_raw(Rs, Ts, ell)
    c.close()
    assert raw == full and bytes(s5) == bytes(summary)


def test_padding_rows_are_never_members(pkg, po):
    """3001 points: the device arrays carry 71 padding rows (3072 rows; NaN features) parked 10 km beyond the cloud's centre along x
    (the cloud handed over first) or y (the other one), 16 m apart (cvo_cloud.hip k_cloud_pad); seven of them share the last
    segment with real rows.  Poses that carry one cloud's real points onto the other's padding rows must find nothing, as
    the restatement, which knows no padding rows, finds nothing."""
    capi = pkg.capi
    x, f, _, _ = pkg.data.synthetic_pair(3001, 3001, seed=43)
    for mode, omode in ((capi.MODE_CVO, 0), (capi.MODE_ACVO, 1), (capi.MODE_MATLAB, 2)):
        ell = 0.15 if mode == capi.MODE_MATLAB else 0.1
        c = _ctx(pkg, capi.default_params(mode), x, f, x, f)
        dev = [c.device_cloud(0), c.device_cloud(1)]
        assert dev[0]["rows"] == 3072 and dev[0]["points"] == 3001
        # the parking rule, from the clouds' corners
        ctr = (0.5 * (x.min(axis=0) + x.max(axis=0))).astype(np.float32)
        for which, axis in ((0, 0), (1, 1)):
            pads = dev[which]["pos"][3001:, :3]
            for q in (0, 3, 40, 70):
                want = ctr.copy()
                want[axis] += np.float32(1.0e4) + np.float32(16.0 * q)
                assert np.allclose(pads[q], want, atol=0.01), (which, q)
            assert np.all(np.isnan(dev[which]["feat"][3001:, :5])) and np.all(np.isnan(dev[which]["pos"][3001:, 3]))
        Rs, Ts = [I3], [Z3]
        for q in (3, 40):   # a padding row that shares a segment with real rows, and one that does not
            # y = z - T: the moving cloud's point 0 lands on the fixed cloud's padding row q ...
            Ts.append((x[0].astype(np.float64) - dev[0]["pos"][3001 + q, :3]).astype(np.float32))
            Rs.append(I3)
            # ... and the moving cloud's padding row q on the fixed cloud's point 0
            Ts.append((dev[1]["pos"][3001 + q, :3].astype(np.float64) - x[0]).astype(np.float32))
            Rs.append(I3)
        got = c.pose_scan(Rs, Ts, ell)
        at_pads = [c.pose_score(Rs[k], Ts[k], ell).nnz for k in range(1, 5)]
        c.close()
        assert got.nnz[0] == got.nnz_fixed == got.nnz_moving and abs(got.cos_angle[0] - 1.0) <= 1e-12
        assert got.nnz[1:].tolist() == [0, 0, 0, 0] == at_pads and not got.inner[1:].any() and got.best == 0
        want = sref.scan(po, omode, ell, x, f, x, f, Rs, Ts)
        assert want["nnz"].tolist() == got.nnz.tolist() and want["nnz_fixed"] == got.nnz_fixed


def test_state_is_the_winners_pose(pkg):
    capi = pkg.capi
    mode, _, (xf, ff, xm, fm), ell = _case(pkg, None, "cvo_3000")
    Rs, Ts = sref.accuracy_poses(*_pose())
    c = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
    s = c.pose_scan(Rs, Ts, ell)
    after = c.flow(ell)
    # every pose empty: the pose stays
    s_none = c.pose_scan(Rs[22:24], Ts[22:24], ell)
    still = c.flow(ell)
    c.close()
    assert s.best >= 0 and s_none.best == -1 and s_none.nnz.tolist() == [0, 0]
    d = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
    d.transform_pcd(Rs[s.best], Ts[s.best])
    fresh = d.flow(ell)
    d.close()
    assert after[8] == fresh[8] == still[8] == s.nnz[s.best] > 0
    for got in (after, still):
        assert abs(got[6] - fresh[6]) <= 2 * sref.gamma(int(fresh[8])) * fresh[6]
    assert abs(s.inner[s.best] - fresh[6]) <= 2 * sref.gamma(int(fresh[8])) * fresh[6]


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_no_side_effects_on_align(pkg, mode_name):
    capi = pkg.capi
    mode = capi.MODE_ACVO if mode_name == "acvo" else capi.MODE_CVO
    xf, ff, xm, fm = pkg.data.synthetic_pair(3000, 3000, seed=31, acvo=mode_name == "acvo")
    Rs, Ts = sref.accuracy_poses(*_pose())
    runs = []
    for with_s in (False, True):
        c = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
        if with_s:
            assert c.pose_scan(Rs, Ts, 0.1).best >= 0
        st = capi.init_state(c.params)
        n, tr = c.align(st, trace_cap=2000)
        runs.append((n, _trace_bits(tr), bytes(st)))
        c.close()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("sc", sref.SCENARIOS, ids=lambda sc: "seed%d" % sc["seed"])
def test_displaced_pair_end_to_end(pkg, po, sc):
    xf, ff, xm, fm = sref.scenario_clouds(pkg, sc)
    ell = sref.SCENARIO_ELL
    grid = sref.scenario_grid()
    # alone: nothing within reach (the oracle: one iteration on an empty member set)
    reg = pkg.Cvo(device=0, stream=_stream())
    reg.set_pcd(xf, ff)
    reg.set_pcd(xm, fm)
    reg.align(score=ell)
    lone_iters, lone_score = reg.num_iterations, reg.score
    reg.close()
    print("alone: iterations", lone_iters, "score", lone_score)
    assert lone_score.nnz == 0 and lone_score.cos_angle == 0.0
    # from the best of the grid
    reg = pkg.Cvo(device=0, stream=_stream())
    reg.set_pcd(xf, ff)
    reg.set_pcd(xm, fm)
    reg.align(init_candidates=grid, scan_ell=ell, score=ell)
    scan, n_it, score, state = reg.scan, reg.num_iterations, reg.score, bytes(reg.state)
    reg.close()
    print("scan best", scan.best, "cos", scan.cos_angle[scan.best], "iterations", n_it, "final cos", score.cos_angle)
    assert scan.count == 344 and scan.nnz[0] == 0
    assert int(np.sum(scan.nnz[1:] == 0)) == sc["empty"]
    assert scan.best == sc["winner"] + 1   # (index 0 of the scanned list is the carried pose, the grid follows)
    assert abs(scan.cos_angle[scan.best] - sc["cos"]) < 5e-4
    assert n_it == sc["iters"]
    assert abs(score.cos_angle - sc["final"]) < 5e-4
    p = po.default_params(po.MODE_CVO)
    so = po.init_state(p)
    so.R[:] = [float(v) for v in grid[0][sc["winner"]].ravel()]
    so.T[:] = [float(v) for v in grid[1][sc["winner"]]]
    n_or, _ = po.align(p, so, xf, ff, xm, fm, search=po.SEARCH_GRID, trace_cap=1)
    assert n_or == n_it and bytes(so) == state


def test_refusals_and_edges(pkg):
    capi = pkg.capi
    p = capi.default_params(capi.MODE_CVO)
    xf, ff, xm, fm = pkg.data.synthetic_pair(2000, 2000, seed=41)
    R, T = _pose()
    Rs, Ts = np.stack([R, I3]), np.stack([T, Z3])
    c = _ctx(pkg, p, xf, ff, xm, fm)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(capi.CvoHipError):
            c.pose_scan(Rs, Ts, bad)
    # no pose: OK, the norms still filled
    s0 = c.pose_scan(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3), np.float32), 0.1)
    sc = c.pose_score(R, T, 0.1)
    assert s0.count == 0 and s0.best == -1 and len(s0.inner) == 0
    assert (s0.self_fixed, s0.self_moving, s0.nnz_fixed, s0.nnz_moving) == (sc.self_fixed, sc.self_moving, sc.nnz_fixed, sc.nnz_moving)
    assert s0.self_fixed > 0 and s0.n_fixed == 2000 and s0.n_moving == 2000
    # null arrays with a pose to score, counts out of range
    L = capi.lib()
    out, summary = (capi.PoseScanEntryC * 2)(), capi.PoseScanC()
    r9, t3 = capi.fptr(np.ascontiguousarray(Rs.reshape(-1, 9))), capi.fptr(np.ascontiguousarray(Ts))
    ell = ctypes.c_float(0.1)
    assert L.cvo_hip_pose_scan(c._ctx, None, t3, 2, ell, out, ctypes.byref(summary)) == -1
    assert L.cvo_hip_pose_scan(c._ctx, r9, None, 2, ell, out, ctypes.byref(summary)) == -1
    assert L.cvo_hip_pose_scan(c._ctx, r9, t3, 2, ell, None, ctypes.byref(summary)) == -1
    assert L.cvo_hip_pose_scan(c._ctx, r9, t3, 2, ell, out, None) == -1
    assert L.cvo_hip_pose_scan(c._ctx, r9, t3, -1, ell, out, ctypes.byref(summary)) == -1
    assert L.cvo_hip_pose_scan(c._ctx, r9, t3, (1 << 20) + 1, ell, out, ctypes.byref(summary)) == -1
    assert L.cvo_hip_pose_scan(c._ctx, r9, t3, 2, ell, out, ctypes.byref(summary)) == 0 and summary.count == 2
    # a non-finite entry
    for arr, at in ((Ts, (1, 2)), (Rs, (0, 1, 1))):
        for v in (float("nan"), float("inf")):
            bad = [Rs.copy(), Ts.copy()]
            bad[0 if arr is Rs else 1][at] = v
            with pytest.raises(capi.CvoHipError, match="non-finite"):
                c.pose_scan(bad[0], bad[1], 0.1)
    # a shard over the whole clouds is the whole registration; a narrower one is refused
    whole, _ = c.pose_scan_raw(Rs, Ts, 0.1)
    c.set_shard(0, len(xf), 0, len(xm))
    assert c.pose_scan_raw(Rs, Ts, 0.1)[0] == whole
    c.set_shard(0, len(xf) // 2, 0, len(xm))
    with pytest.raises(capi.CvoHipError, match="shard"):
        c.pose_scan(Rs, Ts, 0.1)
    c.close()
    # a cloud missing
    c = capi.Context(params=p, device=0, stream=_stream())
    c.set_fixed(xf, ff)
    with pytest.raises(capi.CvoHipError):
        c.pose_scan(Rs, Ts, 0.1)
    c.close()
    # more than 65 536 points in a cloud
    big = pkg.data.synthetic_pair(65537, 2000, seed=3)
    c = _ctx(pkg, p, *big)
    with pytest.raises(capi.CvoHipError, match="65536"):
        c.pose_scan(Rs, Ts, 0.1)
    c.close()
    c = _ctx(pkg, p, big[2], big[3], big[0], big[1])
    with pytest.raises(capi.CvoHipError, match="65536"):
        c.pose_scan(Rs, Ts, 0.1)
    c.close()
    # an all-reduce hook, mailboxes attached
    c = _ctx(pkg, p, xf, ff, xm, fm)
    c.set_allreduce(lambda buf, count, stream: None)
    with pytest.raises(capi.CvoHipError, match="all-reduce"):
        c.pose_scan(Rs, Ts, 0.1)
    c.close()
    c = _ctx(pkg, p, xf, ff, xm, fm)
    c.mailbox_create(0, 1)
    with pytest.raises(capi.CvoHipError, match="mailboxes"):
        c.pose_scan(Rs, Ts, 0.1)
    c.close()


def test_largest_clouds_and_a_second_chunk(pkg):
    """65 536 points a side (1024 segments, 256 blocks per pose) and a call of more poses than one launch takes: the entries
    are those of lone calls, and cvo_hip_pose_score's counts."""
    capi = pkg.capi
    xf, ff, xm, fm = pkg.data.synthetic_pair(65536, 65536, seed=11)
    R, T = _pose()
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    raw, s = c.pose_scan_raw(np.stack([R, I3, I3]), np.stack([T, Z3, Z3 + np.float32(90.0)]), 0.1)
    sc = c.pose_score(R, T, 0.1)
    c.close()
    e = _entries(pkg, raw)
    assert e["nnz"][0] == sc.nnz > 0 and e["nnz"][2] == 0 and s.nnz_fixed == sc.nnz_fixed
    assert abs(e["inner"][0] - sc.inner) <= 2 * sref.gamma(sc.nnz) * sc.inner
    xf, ff, xm, fm = pkg.data.synthetic_pair(700, 900, seed=12)
    c = _ctx(pkg, capi.default_params(capi.MODE_CVO), xf, ff, xm, fm)
    Rs, Ts = sref.accuracy_poses(R, T)
    reps = 4096 // 25 + 2
    many, sm = c.pose_scan_raw(np.tile(Rs, (reps, 1, 1)), np.tile(Ts, (reps, 1)), 0.1)
    few, sf = c.pose_scan_raw(Rs, Ts, 0.1)
    c.close()
    assert sm.count == 25 * reps > 4096 and many == few * reps and sm.best == sf.best


def test_cpp_mirror_matches_python(pkg, desk, tmp_path):
    lib = os.path.join(ROOT, "cvo-rgbd_amd", "csrc")
    exe = str(tmp_path / "cvo_scan_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "cvo_scan_demo.cpp"), "-L", lib, "-lcvo_hip",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    frames = [(desk["xyz%d" % k], pkg.data.cvo_features(desk["rgb%d" % k])) for k in range(2)]
    Rs, Ts = sref.accuracy_poses(*_pose())
    ell = np.float32(0.1)
    path = str(tmp_path / "scan.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(frames)))
        for x, f in frames:
            fh.write(struct.pack("<i", len(x)))
            fh.write(np.ascontiguousarray(x, np.float32).tobytes())
            fh.write(np.ascontiguousarray(f, np.float32).tobytes())
        fh.write(struct.pack("<i", len(Rs)))
        fh.write(np.ascontiguousarray(Rs, np.float32).tobytes())
        fh.write(np.ascontiguousarray(Ts, np.float32).tobytes())
        fh.write(struct.pack("<f", ell))
    lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    c = _ctx(pkg, pkg.capi.default_params(pkg.capi.MODE_CVO), *frames[0], *frames[1])
    s = c.pose_scan(Rs, Ts, ell)
    c.close()
    tok = dict((ln.split()[0], ln.split()[1]) for ln in lines if not ln.startswith("pose "))
    for k in ("count", "best", "nnz_fixed", "nnz_moving", "n_fixed", "n_moving"):
        assert int(tok[k]) == getattr(s, k), k
    for k in ("self_fixed", "self_moving", "ell"):
        assert float.fromhex(tok[k]) == getattr(s, k), k
    poses = [ln.split() for ln in lines if ln.startswith("pose ")]
    assert len(poses) == 25
    for k, t in enumerate(poses):
        assert int(t[1]) == k and int(t[2]) == s.nnz[k]
        assert (float.fromhex(t[3]), float.fromhex(t[4]), float.fromhex(t[5])) == (s.inner[k], s.cos_angle[k], s.mean_d2[k]), k


def test_one_scan_is_faster_than_lone_scores(pkg):
    """The safe half of the speed bar (tools/pose_scan_bench.py measures the rest): one scan of 256 poses takes less time
    than 256 lone cvo_hip_pose_score calls, medians of 5, warm norm caches."""
    capi = pkg.capi
    mode, _, (xf, ff, xm, fm), ell = _case(pkg, None, "cvo_3000")
    R25, T25 = sref.accuracy_poses(*_pose())
    Rs, Ts = np.tile(R25, (11, 1, 1))[:256], np.tile(T25, (11, 1))[:256]
    c = _ctx(pkg, capi.default_params(mode), xf, ff, xm, fm)
    c.pose_scan(Rs, Ts, ell)
    c.pose_score(Rs[0], Ts[0], ell)
    t_scan, t_score = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        c.pose_scan_raw(Rs, Ts, ell)
        t1 = time.perf_counter()
        for k in range(256):
            c.pose_score_raw(Rs[k], Ts[k], ell)
        t2 = time.perf_counter()
        t_scan.append(t1 - t0)
        t_score.append(t2 - t1)
    c.close()
    print("scan of 256: %.3f ms, 256 scores: %.3f ms" % (1e3 * np.median(t_scan), 1e3 * np.median(t_score)))
    assert np.median(t_scan) < np.median(t_score)
