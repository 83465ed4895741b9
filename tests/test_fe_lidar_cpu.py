"""No GPU: the restatement of the LiDAR contract (tests/fe_lidar_ref.py) against itself -- the vectorised cull against
the per-pixel loop, a point and a window by hand -- what the made scans are for (they reach every skip rule and both
flags, with the counts stated; each mutant of tests/fe_lidar_mutants.py is told from the restatement by some made scan
at every point of the grid at which its error can show), the struct, cvo_fe_check_lidar with one refusal per reason and
the other host-only refusals of the library, and the parameters of the layers above."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import fe_lidar_mutants as M
import fe_lidar_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = K.SIZES[0]


def _same(got, want):
    return all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got[:3], want[:3]))


# ---- 1. two statements of the contract ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["threshold", "clutter-4097", "pile", "skips"])
def test_the_vectorised_cull_equals_the_loop(name):
    for grid in ((0, 7, 0, 0.25), (1, 0, 7, 0.25), (2, 3, 1, 0.25), (1, 7, 7, 0.25), (1, 7, 7, 0.0), (3, 0, 0, 0.25)):
        points, s, cam, w, h, (P, P0, flags, hits, occluded) = K.made(name, SMALL, grid)
        loop = K.cull_loop(P0, s)
        assert P.dtype == np.uint16 and flags.dtype == np.uint8 and P.shape == flags.shape == (h, w)
        assert loop[0].tobytes() == P.tobytes() and loop[1].tobytes() == flags.tobytes(), (name, grid)


def test_a_point_and_a_window_by_hand():
    """fx 64, cx 48, scale 1024: (0.25, 0, 2) lands on u = 64 * 0.125 + 48 = 56 with q 2048; u = 2.5 is pixel 2 and
    3.5 pixel 4; beside a 4000 a 5000 stays and a 5001 goes, at rel 0.25"""
    cam = K.exact_cam(96, 64)
    s = K.setting((0, 0, 0, 0.0))
    P0, why = K.project(np.array([[0.25, 0.0, 2.0]], np.float32), s, cam, 96, 64)
    assert np.count_nonzero(P0) == 1 and P0[32, 56] == 2048 and list(why) == [K.WROTE]
    pts = K.lift([2.5, 3.5, 10.5], [0.5, 1.5, 7.0], [1024, 1032, 1040], cam)
    P0, _ = K.project(pts, s, cam, 96, 64)
    assert P0[0, 2] == 1024 and P0[2, 4] == 1032 and P0[7, 10] == 1040 and np.count_nonzero(P0) == 3
    P0, _ = K.project(pts, K.setting((1, 0, 0, 0.0)), cam, 96, 64)
    # (the splat at the top border is cut to 3 x 2; the two first splats share pixel (3, 1), and the nearer wins)
    assert np.count_nonzero(P0) == 6 + 9 - 1 + 9 and P0[1, 3] == 1024
    plane = np.zeros((3, 20), np.uint16)
    plane[1, 2], plane[1, 5], plane[1, 12], plane[1, 15] = 4000, 5000, 4000, 5001
    P, flags = K.cull(plane, K.setting((0, 3, 0, 0.25)))
    assert P[1, 5] == 5000 and P[1, 15] == 0 and flags[1, 15] == K.HIT | K.OCCLUDED and flags[1, 5] == K.HIT
    assert P[1, 2] == P[1, 12] == 4000 and np.count_nonzero(flags) == 4
    assert K.cull(plane, K.setting((0, 2, 7, 0.25)))[0][1, 15] == 5001      # out of the window's reach
    assert K.cull(plane, K.setting((0, 3, 0, 0.0)))[0][1, 15] == 5001       # no test


def test_the_exact_camera_is_exact():
    """the points of `halves` land on their ties: u and v of the arithmetic are the positions they were made for"""
    for w, h in K.SIZES:
        cam = np.asarray(K.exact_cam(w, h), np.float32)
        p = K.scan_halves(w, h)
        u = cam[1] * (p[:, 0] / p[:, 2]) + cam[3]
        v = cam[2] * (p[:, 1] / p[:, 2]) + cam[4]
        assert u.dtype == np.float32 and (u * 2 == np.rint(u * 2)).all() and (v * 2 == np.rint(v * 2)).all()
        for frac in (u - np.floor(u), v - np.floor(v)):
            assert np.count_nonzero(frac == 0.5) >= len(p) // 3 and np.count_nonzero(frac == 0) >= len(p) // 3
        ties = np.floor(u[u != np.floor(u)]).astype(int)
        assert (ties % 2 == 0).any() and (ties % 2 == 1).any()            # ties that go down and ties that go up


# ---- 2. what the made scans reach ---------------------------------------------------------------------

def _counts(why):
    return {int(k): int(n) for k, n in zip(*np.unique(why, return_counts=True))}


@pytest.mark.parametrize("size", K.SIZES, ids=["%dx%d" % s for s in K.SIZES])
def test_the_made_scans_reach_every_skip_rule(size):
    grid = (0, 0, 0, 0.0)
    points, s, cam, w, h = K.case("skips", size, grid)
    got = _counts(K.project(points, s, cam, w, h)[1])
    assert got == {k: n for k, n in K.SKIP_COUNTS.items() if n}, got
    P0 = K.project(points, s, cam, w, h)[0]
    assert {1, 65535} <= set(np.unique(P0)) and np.count_nonzero(P0) == 7
    points, s, cam, w, h = K.case("ranges", size, grid)
    assert (s.min_range, s.max_range) == K.RANGE_LIMITS
    got = _counts(K.project(points, s, cam, w, h)[1])
    assert got == K.RANGE_COUNTS, got
    # the borders: at splat 0 the 4 x 8 points one to four pixels outside and the five far outside write nothing, the
    # eight on the border pixels write; at splat k the points up to k outside write too
    points, s, cam, w, h = K.case("borders", size, grid)
    for splat in K.SPLATS:
        why = K.project(points, K.setting((splat, 0, 0, 0.0)), cam, w, h)[1]
        assert _counts(why) == {K.WROTE: 8 * (splat + 1), K.OUTSIDE: 45 - 8 * (splat + 1)}, splat
    # far outside: clamped to 8 pixels outside, not wrapped to the other side and not written
    assert (K.project(points[-5:], K.setting((3, 0, 0, 0.0)), cam, w, h)[1] == K.OUTSIDE).all()


@pytest.mark.parametrize("size", K.SIZES, ids=["%dx%d" % s for s in K.SIZES])
def test_the_made_scans_reach_both_flags(size):
    """the threshold at equality and one above it, at splat 0 where no pair reaches another: of the seven pairs with a
    5001 a window drops those it reaches; no 5000 is ever dropped; (8, 8) is out of every window's reach"""
    reach = {(0, 0): 0, (7, 0): 2, (0, 7): 1, (3, 1): 1, (7, 7): 6}
    for (rx, ry), n in reach.items():
        assert n == sum(1 for dx, dy in K.THRESHOLD_PAIRS if dx <= rx and dy <= ry)
        P, P0, flags, hits, occluded = K.made("threshold", size, (0, rx, ry, 0.25))[5]
        assert (hits, occluded) == (30, n) and set(np.unique(P0[flags == K.HIT | K.OCCLUDED])) <= {5001}
        assert np.count_nonzero(P == 5000) == 7 and np.count_nonzero(P == 65535) == 1
        assert K.made("threshold", size, (0, rx, ry, 0.0))[5][4] == 0
    # the clutter: at 4097 points both images are dense enough for every window to drop pixels; some 256 points on
    # 127 x 193 pixels mostly have no neighbour in reach, and nothing is asked of them but to be there
    for n in K.COUNTS[2:]:
        for grid in K.GRID:
            hits, occluded = K.made("clutter-%d" % n, size, grid)[5][3:]
            assert hits >= 100 and (M.CULLS(grid) or occluded == 0), (n, grid, hits, occluded)
            assert n < 4097 or (occluded >= 5) == M.CULLS(grid), (n, grid, hits, occluded)
    assert K.made("clutter-0", size, (1, 7, 7, 0.25))[5][3:] == (0, 0)
    assert K.made("clutter-1", size, (1, 7, 7, 0.25))[5][3:] == (9, 0)
    # many points on one pixel: the nearest of them, whatever the order
    points, s, cam, w, h, (P, P0, flags, hits, occluded) = K.made("pile", size, (0, 0, 0, 0.0))
    assert P0[17, 31] == 1024 * points[:60, 2].min() and hits < len(points) // 2
    assert _same(K.lidar(K.shuffled(points), s, cam, w, h), (P, P0, flags))


# ---- 3. the mutants -----------------------------------------------------------------------------------

TELLERS = ["halves", "borders", "skips", "ranges", "pile", "threshold", "chains", "clutter-257", "clutter-4097"]


@pytest.mark.parametrize("name", list(M.PLAIN))
def test_every_mutant_is_told_at_every_setting(name):
    """at every point of the grid at which the mutant's error can show some made scan gives other bytes than the
    restatement, at both image sizes; where it cannot show the mutant IS the restatement"""
    mutant, shows = M.PLAIN[name]
    if name == "in_place":            # (a loop over the pixels: the smaller image)
        sizes = K.SIZES[:1]
    else:
        sizes = K.SIZES
    for size in sizes:
        for grid in K.GRID:
            told = [c for c in TELLERS if not _same(mutant(*K.case(c, size, grid)), K.made(c, size, grid)[5])]
            assert bool(told) == bool(shows(grid)), (name, size, grid, told)


@pytest.mark.parametrize("mutant, case, grid", [
    (M.half_up, "halves", (0, 0, 0, 0.0)),               # a tie on an even pixel goes up
    (M.truncated, "halves", (0, 0, 0, 0.0)),             # a tie on an odd pixel stays down
    (M.farthest_wins, "pile", (0, 0, 0, 0.0)),
    (M.splat_wraps, "borders", (0, 0, 0, 0.0)),          # a nearest pixel left of the image is the row above's last
    (M.splat_wraps, "borders", (2, 0, 0, 0.0)),
    (M.range_on_norm, "ranges", (0, 0, 0, 0.0)),         # off the axis |Q| is beyond a limit and Q.z inside
    (M.raw_depth, "clutter-257", (0, 0, 0, 0.0)),        # only a scan under a mount has another z than Q.z
    (M.zeros_counted, "threshold", (0, 7, 0, 0.25)),     # every pixel beside an empty one is dropped
    (M.max_is_none, "threshold", (0, 0, 0, 0.0)),
    (M.max_is_none, "skips", (0, 0, 0, 0.0)),
    (M.at_equality, "threshold", (0, 3, 1, 0.25)),       # the 5000 three to the right, one down
    (M.window_swapped, "threshold", (0, 7, 0, 0.25)),
    (M.window_swapped, "threshold", (0, 3, 1, 0.25)),
    (M.in_place, "clutter-4097", (1, 7, 7, 0.25)),
    (M.in_place, "chains", (0, 7, 0, 0.25)),             # C stays when B is gone before C is looked at
    (M.in_place, "chains", (3, 3, 1, 0.25)),
])
def test_a_scan_tells_the_mutant(mutant, case, grid):
    assert not _same(mutant(*K.case(case, SMALL, grid)), K.made(case, SMALL, grid)[5])


def test_only_a_mount_shows_the_raw_depth_and_only_a_window_the_cull():
    """the exact scans have R = I and T = 0: their z IS Q.z.  Without a window nothing of the cull shows."""
    for c in TELLERS[:7]:
        assert _same(M.raw_depth(*K.case(c, SMALL, (1, 0, 0, 0.0))), K.made(c, SMALL, (1, 0, 0, 0.0))[5])
    for name in ("zeros_counted", "at_equality", "in_place", "tile_cut_64x16"):
        for grid in ((1, 0, 0, 0.25), (1, 7, 7, 0.0)):
            assert _same(M.PLAIN[name][0](*K.case("clutter-4097", SMALL, grid)), K.made("clutter-4097", SMALL, grid)[5])


@pytest.mark.parametrize("tile", M.TILES, ids=["%dx%d" % t for t in M.TILES])
def test_the_clutter_tells_a_lost_halo(tile):
    """tiles of 32 x 8, 64 x 4, 16 x 16 and the kernel's 64 x 16: both images have a seam of each inside, both ways; and
    it is the seams that tell: away from them the mutant is the restatement"""
    for size in K.SIZES:
        assert tile[0] < size[0] and tile[1] < size[1]
        for grid in ((1, 7, 0, 0.25), (1, 0, 7, 0.25), (0, 3, 1, 0.25), (2, 7, 7, 0.25)):
            want = K.made("clutter-4097", size, grid)[5]
            got = M.tile_cut(*tile)(*K.case("clutter-4097", size, grid))
            ys, xs = np.nonzero(got[0] != want[0])
            rx, ry = grid[1], grid[2]
            near_x = (xs % tile[0] < rx) | (xs % tile[0] >= tile[0] - rx)
            near_y = (ys % tile[1] < ry) | (ys % tile[1] >= tile[1] - ry)
            assert len(ys) > 0 and (near_x | near_y).all(), (size, grid)
    assert K.TILE in M.TILES


def test_alternating_counts_tell_a_stale_count():
    """300, 0, 4097, 1 points on one context: with the count of the frame before every frame has other bytes"""
    w, h = SMALL
    s, cam = K.setting((1, 7, 1, 0.25), **K.MOUNT), K.plain_cam(w, h)
    scans = K.frame_scans(w, h, s, cam)
    assert [len(p) for p in scans] == list(K.ALTERNATING)
    want = [K.lidar(p, s, cam, w, h) for p in scans]
    stale = M.stale_counts(scans, s, cam, w, h, 4200)
    for k in range(len(scans)):
        assert not _same(stale[k], want[k]), k
    assert want[1][3] == 0 and want[3][3] == 9 and want[0][3] > 300 and want[2][4] >= 5
    for k in range(len(scans)):
        for j in range(k):
            assert want[k][0].tobytes() != want[j][0].tobytes()


# ---- 4. what is accepted, and the layers above -------------------------------------------------------

def test_the_struct_and_the_constants(pkg):
    F = pkg.frontend
    assert C.sizeof(F.Lidar) == 80
    offsets = {name: getattr(F.Lidar, name).offset for name, _ in F.Lidar._fields_}
    assert offsets == {"max_points": 0, "splat": 4, "R": 8, "T": 44, "min_range": 56, "max_range": 60, "occl_rel": 64,
                       "occl_rx": 68, "occl_ry": 72, "pad_": 76}
    l = F.Lidar(1000, 2, K.MOUNT_R, K.MOUNT_T, 0.5, 80.0, 0.25, 7, 1)
    want = (np.array([1000, 2], np.int32).tobytes() + np.array(K.MOUNT_R + K.MOUNT_T + (0.5, 80.0, 0.25), np.float32).tobytes() +
            np.array([7, 1, 0], np.int32).tobytes())
    assert bytes(l) == want and l == F.Lidar(1000, 2, K.MOUNT_R, K.MOUNT_T, 0.5, 80.0, 0.25, 7, 1) != F.Lidar(1000, 2)
    assert repr(F.Lidar(5)).startswith("Lidar(max_points=5, splat=0, R=(1.0, 0.0, 0.0, 0.0, 1.0,")
    assert bytes(F.Lidar(5, pad_=3))[76:] == np.array([3], np.int32).tobytes()
    assert (F.STAGE_LIDAR_DEPTH, F.STAGE_LIDAR, F.LIDAR_HIT, F.LIDAR_OCCLUDED) == (26, 27, K.HIT, K.OCCLUDED) == (26, 27, 1, 2)
    assert (F.STAGE_UNFILTERED_DEPTH, F.STAGE_MEDIAN) == (24, 25)
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    for pattern in (r"CVO_FE_STAGE_LIDAR_DEPTH = 26\b", r"CVO_FE_STAGE_LIDAR = 27\b", r"CVO_FE_LIDAR_HIT = 1\b",
                    r"CVO_FE_LIDAR_OCCLUDED = 2\b", r"THE LIDAR CONTRACT", r"\} cvo_fe_lidar;\s*/\* 80 bytes, no padding \*/"):
        assert re.search(pattern, text), pattern
    for name in ("cvo_fe_check_lidar", "cvo_fe_set_lidar", "cvo_fe_get_lidar", "cvo_fe_submit_lidar",
                 "cvo_fe_create_pointcloud_lidar", "cvo_fe_project_points"):
        assert name in F.SYMBOLS and re.search(r"\bint %s\(" % name, text), name
    hip = open(os.path.join(ROOT, "include", "cvo_hip.h")).read()
    assert "lidar" not in hip.lower()


def test_check_lidar(pkg):
    """host only, through the library: the one statement of what is accepted, one refusal per reason"""
    F = pkg.frontend
    for s in K.good_lidars():
        assert F.check_lidar(F.Lidar(*s)), s
    for grid in K.GRID:
        assert F.check_lidar(K.to_struct(F, K.setting(grid, **K.MOUNT)))
    bad = K.bad_lidars()
    assert len(bad) == 19
    for reason, s in bad.items():
        assert not F.check_lidar(F.Lidar(*s)), reason
    assert not F.check_lidar(None)
    # a rotation within 1e-3 is one; beyond it is none
    near = tuple(float(v) for v in (np.asarray(K.IDENTITY) + np.array([0, 4e-4, 0, 0, 0, 0, 0, 0, 0])))
    far = tuple(float(v) for v in (np.asarray(K.IDENTITY) + np.array([0, 2e-3, 0, 0, 0, 0, 0, 0, 0])))
    assert F.check_lidar(F.Lidar(5, R=near)) and not F.check_lidar(F.Lidar(5, R=far))
    L = F.lib()
    out, isset = F.Lidar(7, 2), C.c_int(7)
    assert L.cvo_fe_set_lidar(None, C.byref(out)) != 0
    assert L.cvo_fe_get_lidar(None, C.byref(out), C.byref(isset)) != 0 and (out.max_points, out.splat, isset.value) == (7, 2, 7)
    assert L.cvo_fe_submit_lidar(None, None, 0, None, 16, 0, 4, 1) != 0


def test_project_points_refuses_before_it_touches_a_device(pkg):
    """the host-only refusals of the context-free entry: they come before any device is touched"""
    F = pkg.frontend
    L = F.lib()
    pts = np.ones((4, 4), np.float32)
    plane = np.full((4, 4), 7, np.uint16)
    hits, occl = C.c_int(-5), C.c_int(-6)
    good, cam = F.Lidar(1), np.array([1000.0, 50.0, 50.0, 2.0, 2.0], np.float32)
    u16p, fp = C.POINTER(C.c_uint16), C.POINTER(C.c_float)

    def call(points=pts.ctypes.data, stride=16, n=4, l=good, c=cam, w=4, h=4, out=plane, nh=hits, no=occl):
        return L.cvo_fe_project_points(0, points, stride, n, None if l is None else C.byref(l),
                                       None if c is None else c.ctypes.data_as(fp), w, h,
                                       None if out is None else out.ctypes.data_as(u16p), None, None,
                                       None if nh is None else C.byref(nh), None if no is None else C.byref(no))

    bad_cams = [np.array(v, np.float32) for v in ([0, 50, 50, 2, 2], [1000, 0, 50, 2, 2], [1000, 50, -1, 2, 2],
                                                   [1000, 50, 50, np.nan, 2], [np.inf, 50, 50, 2, 2])]
    refused = [call(points=None), call(stride=8), call(stride=14), call(n=-1), call(n=K.MAX_POINTS + 1), call(l=None),
               call(c=None), call(w=0), call(h=0), call(w=8193), call(h=8193), call(out=None), call(nh=None), call(no=None),
               call(l=F.Lidar(1, 4)), call(l=F.Lidar(1, occl_rx=8)), call(l=F.Lidar(1, pad_=1))]
    refused += [call(c=c) for c in bad_cams]
    assert all(rc == -1 for rc in refused), refused
    assert (hits.value, occl.value) == (-5, -6) and (plane == 7).all()
    # max_points is not read: 0 there is no reason
    assert call(l=F.Lidar(0), w=0) == -1 and call(l=F.Lidar(0)) in (0, -5)


def test_the_drivers_have_the_parameter(pkg):
    F = pkg.frontend
    p = inspect.signature(F.run_frames).parameters
    assert "lidar" in p and p["lidar"].default is None
    p = inspect.signature(F.run_lidar_directory).parameters
    assert list(p)[:4] == ["registration", "folder", "dataset_seq", "lidar"]
    assert (p["image"].default, p["scans"].default, p["times"].default) == ("image_2", "velodyne", "times.txt")
    same = set(inspect.signature(F.run_stereo_directory).parameters) - {"stereo", "left", "right", "stereo_rig", "stereo_paths",
                                                                          "stereo_speckle"}
    assert same <= set(p), same - set(p)
    for name in ("set_lidar", "lidar", "create_pointcloud_lidar", "submit_lidar"):
        assert callable(getattr(F.PcdGenerator, name)), name
    assert callable(F.project_points) and callable(F.check_lidar)
    hpp = open(os.path.join(ROOT, "include", "cvo.hpp")).read()
    for decl in ("void set_lidar(const cvo_fe_lidar &", "void clear_lidar();", "void set_pcd_lidar(const int dataset_seq,",
                 "void run_cvo_lidar(const int dataset_seq,"):
        assert decl in hpp, decl


def test_run_lidar_directory_reads_the_kitti_layout(pkg, tmp_path):
    """the file side: times.txt, image_2/%06d.png and velodyne/%06d.bin of four float32 per record reach run_frames as
    (name, bgr, n x 4 points), with the pass-through settings"""
    from PIL import Image
    F = pkg.frontend
    (tmp_path / "image_2").mkdir()
    (tmp_path / "velodyne").mkdir()
    rng = np.random.RandomState(3)
    rgb = [rng.randint(0, 255, (8, 12, 3)).astype(np.uint8) for _ in range(3)]
    scans = [rng.rand(5 + k, 4).astype(np.float32) for k in range(3)]
    (tmp_path / "times.txt").write_text("0.0\n0.1\n0.2\n")
    for k in range(3):
        Image.fromarray(rgb[k]).save(str(tmp_path / "image_2" / ("%06d.png" % k)))
        scans[k].tofile(str(tmp_path / "velodyne" / ("%06d.bin" % k)))
    seen = {}

    def fake(registration, frames, dataset_seq, **kw):
        seen["frames"], seen["kw"], seen["seq"] = list(frames), kw, dataset_seq
        return len(seen["frames"])

    real, F.run_frames = F.run_frames, fake
    try:
        lid = F.Lidar(100, 1)
        assert F.run_lidar_directory("reg", str(tmp_path), 4, lid, limit=2, select_mode=F.SELECT_DEPTH,
                                     depth_median=F.DepthMedian(1, 3)) == 2
    finally:
        F.run_frames = real
    assert [f[0] for f in seen["frames"]] == ["0.0", "0.1"] and seen["seq"] == 4
    for k, (name, bgr, pts) in enumerate(seen["frames"]):
        assert np.array_equal(bgr, rgb[k][:, :, ::-1]) and pts.dtype == np.float32 and np.array_equal(pts, scans[k])
    kw = seen["kw"]
    assert kw["lidar"] is lid and kw["select_mode"] == F.SELECT_DEPTH and kw["depth_median"] == F.DepthMedian(1, 3)
    assert kw["camera"] is None and kw["depth_gate"] is None and kw["mask"] is None and kw["generator"] is None
