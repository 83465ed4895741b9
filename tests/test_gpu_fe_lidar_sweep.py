"""GPU: motion compensation of a spinning scan (cvo_fe_set_lidar_sweep, cvo_fe_set_lidar_motion,
cvo_fe_project_points_sweep; the sweep contract of include/cvo_frontend.h): the instances of k_fe_lidar_project of
csrc/cvo_lidar.hip against the restatement tests/fe_lidar_sweep_ref.py -- the phase and p' of every point by bits, the
plane, the plane before culling, the flags and both counts by bytes, in all three modes, at every count around the block
of 256, both image sizes, strides 16 and 32 with the time word at offset 12 and at the record's end, the hostile records
among them.  On a context: frames whose twist and count both alternate, with and without captured graphs (a stale twist
or a stale graph would show), the cloud by bits against the front-end oracle, a zero twist against a context without a
sweep, the sweep set, changed and cleared between frames, the stages behind the plane, the refusals, run_frames and the
C++ objects above.  What the scans reach, and which errors they would show, is asserted in
tests/test_fe_lidar_sweep_cpu.py."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_gate_ref as G
import fe_lidar_ref as K
import fe_lidar_sweep_ref as S
import fe_median_ref as KM
import test_gpu_fe_lidar as TL
from fe_gpu_common import ROOT, _demo_lines, _device_path_lines, _same_cloud

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = {"time_f32": S.TIME_F32, "time_u32": S.TIME_U32, "azimuth": S.AZIMUTH}


def _bits_equal(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    a, b = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("%s differs in bits at %d places, first at %s: %r against %r"
                             % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _nan_as_one(a):
    """every NaN as the quiet NaN the kernel writes: the restatement's may carry another payload"""
    return np.where(np.isnan(a), f32(np.nan), a).astype(f32)


def _stand_alone(F, rec, s, cam, w, h, sw, twist, want, what):
    got = F.project_points_sweep(rec, K.to_struct(F, s), cam, w, h, S.to_struct(F, sw), twist)
    _bits_equal(_nan_as_one(got[5]), _nan_as_one(want[5]), "the phase of %s" % (what,))
    _bits_equal(_nan_as_one(got[6]), _nan_as_one(want[6]), "p' of %s" % (what,))
    for k, part in enumerate(("P", "P0", "the flags")):
        TL._differ(got[k], want[k], "%s of %s" % (part, what))
    assert got[3:5] == tuple(want[3:5]), (what, got[3:5], want[3:5])


# ---- 1. the stand-alone entry ------------------------------------------------------------------------

@pytest.mark.parametrize("mode_name", list(MODES))
def test_project_points_sweep_on_the_made_scans(pkg, mode_name):
    """every count around the block of 256, both image sizes, every layout of the record; the hostile records are the
    first of every scan (a NaN and an infinite time, times outside the sweep, 0xFFFFFFFF, s == s_ref, x = y = 0, the
    axes and the ties)"""
    F = pkg.frontend
    mode = MODES[mode_name]
    layouts = S.LAYOUTS if mode != S.AZIMUTH else ((3, 0), (4, 3))
    for size in S.SIZES:
        for n in S.COUNTS:
            for layout in layouts:
                c = S.made(mode, n, size, layout)
                _stand_alone(F, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], (mode_name, size, n, layout))
        print(mode_name, size, "hits", c[7][3], "occluded", c[7][4], "without a phase", int(np.isnan(c[7][5]).sum()))


@pytest.mark.parametrize("mode_name", list(MODES))
def test_project_points_sweep_at_the_cap_and_under_other_settings(pkg, mode_name):
    """|w| = 1 exactly with s_ref at an end (the series at t2 = 1), a pure translation, no twist, the other direction,
    other settings of the scan source"""
    F = pkg.frontend
    mode = MODES[mode_name]
    for kw in (dict(twist="unit", s_ref=0.0), dict(twist="unit", s_ref=1.0), dict(twist="shift"), dict(twist="zero"),
               dict(direction=-1), dict(grid=(0, 0, 0, 0.0)), dict(grid=(3, 7, 7, 0.25), twist="unit")):
        if "direction" in kw and mode != S.AZIMUTH:
            continue
        c = S.made(mode, 4097, S.SIZES[1], **kw)
        _stand_alone(F, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], (mode_name, kw))
    # without a sweep the entry is cvo_fe_project_points, and with a zero twist the planes are its planes
    c = S.made(mode, 4097, S.SIZES[0], twist="zero")
    alive = np.isfinite(c[7][5])
    plain = F.project_points(np.where(alive[:, None], c[0][:, :3], f32(np.nan)), K.to_struct(F, c[1]), c[2], c[3], c[4])
    for k in range(3):
        TL._differ(plain[k], c[7][k], "a zero twist against no sweep")


def test_phase_and_moved_may_be_null(pkg):
    F = pkg.frontend
    c = S.made(S.TIME_U32, 257, S.SIZES[0])
    rec, s, cam, w, h, sw, twist, want = c
    plane, hits, occl = np.zeros((h, w), np.uint16), C.c_int(-1), C.c_int(-1)
    camf, fp = np.asarray(cam, f32), C.POINTER(C.c_float)
    phase = np.zeros(len(rec), f32)
    for ph in (None, phase):
        rc = F.lib().cvo_fe_project_points_sweep(
            0, rec.ctypes.data, 16, len(rec), C.byref(K.to_struct(F, s)), camf.ctypes.data_as(fp), w, h,
            plane.ctypes.data_as(C.POINTER(C.c_uint16)), None, None, C.byref(hits), C.byref(occl),
            C.byref(S.to_struct(F, sw)), twist.ctypes.data_as(fp), None if ph is None else ph.ctypes.data_as(fp), None)
        assert rc == 0 and plane.tobytes() == want[0].tobytes() and (hits.value, occl.value) == tuple(want[3:5])
    _bits_equal(_nan_as_one(phase), _nan_as_one(want[5]), "the phase alone")


# ---- 2. frames on a context --------------------------------------------------------------------------

def _frame_records(F, w, h, seq, s, sw, counts=S.FRAME_COUNTS, seed=80, layout=(4, 3)):
    cam = TL._table(F, seq)
    return [S.records_of(K.scan_clutter(w, h, n, seed + k, s, cam), sw, layout) for k, n in enumerate(counts)]


def _sweep_frame(gen, F, bgr, rec, s, seq, sw, twist, ftype=None):
    """one frame under the sweep and the twist: the planes by bytes, the cloud by bits against the oracle on P"""
    ftype = F.FEATURES_RGB if ftype is None else ftype
    h, w = bgr.shape[:2]
    want = S.lidar_sweep(rec, s, TL._table(F, seq), w, h, sw, twist)
    gen.set_lidar_motion(twist)
    assert np.array_equal(gen.lidar_motion(), np.asarray(twist, f32))
    cloud = gen.create_pointcloud_lidar(bgr, rec, seq, ftype)
    TL._planes_equal(gen, F, want)
    TL._cloud_equal(gen, F, cloud, bgr, want[0], seq, ftype)
    return cloud, want


def _alternating(pkg, mode=S.TIME_F32):
    """twists and counts that both alternate on one context, twice over: every frame by bytes"""
    F = pkg.frontend
    w, h = 96, 64
    seq = TL.SEQS[(w, h)]
    bgr = G.frame(w, h, 72)
    s = K.setting((1, 7, 1, 0.25), **K.MOUNT)
    sw = S.sweep_of(mode)
    scans = _frame_records(F, w, h, seq, s, sw)
    gen = TL._generator(pkg, w, h)
    gen.set_lidar(K.to_struct(F, s, max_points=4097))
    gen.set_lidar_sweep(S.to_struct(F, sw))
    assert gen.lidar_sweep() == S.to_struct(F, sw) and not gen.lidar_motion().any()
    sizes, planes = [], []
    for k in range(2 * len(scans)):
        cloud, want = _sweep_frame(gen, F, bgr, scans[k % 4], s, seq, sw, S.TWISTS[S.FRAME_TWISTS[k % 4]])
        sizes.append((want[3], len(cloud[0])))
        planes.append(want[0].tobytes())
    # and the same scan under another twist is another plane: the twist is not captured
    _, other = _sweep_frame(gen, F, bgr, scans[2], s, seq, sw, S.TWISTS["turn"])
    assert other[0].tobytes() != planes[2]
    gen.close()
    assert sizes[1] == (0, 0) and sizes[0][0] > 300 and sizes[:4] == sizes[4:]
    return sizes


@pytest.mark.parametrize("mode_name", list(MODES))
def test_twists_and_counts_alternate_on_one_context(pkg, mode_name):
    """the twist travels in the header with the count and the points: a captured graph carries it"""
    assert os.environ.get("CVO_FE_NO_GRAPH") is None
    _alternating(pkg, MODES[mode_name])


def test_twists_and_counts_alternate_without_captured_graphs():
    """... and in a session that has CVO_FE_NO_GRAPH in its environment from the start (the library reads it once)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import __graft_entry__ as ge, test_gpu_fe_lidar_sweep as T\n"
            "print('sizes', T._alternating(ge.load_package()))\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, CVO_FE_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "sizes [" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_a_zero_twist_is_a_context_without_a_sweep(pkg):
    """byte for byte and bit for bit, frame by frame"""
    F = pkg.frontend
    w, h = 96, 64
    seq = TL.SEQS[(w, h)]
    bgr = G.frame(w, h, 72)
    s = K.setting((1, 7, 1, 0.25), **K.MOUNT)
    sw = S.sweep_of(S.AZIMUTH)
    scans = [r[np.isfinite(r[:, :3]).all(axis=1)] for r in _frame_records(F, w, h, seq, s, sw)]
    plain, swept = TL._generator(pkg, w, h), TL._generator(pkg, w, h)
    for gen in (plain, swept):
        gen.set_lidar(K.to_struct(F, s, max_points=4097))
    swept.set_lidar_sweep(S.to_struct(F, sw))
    for rec in scans + scans:
        a, b = plain.create_pointcloud_lidar(bgr, rec, seq), swept.create_pointcloud_lidar(bgr, rec, seq)
        assert _same_cloud(a, b)
        for stage in (F.STAGE_LIDAR_DEPTH, F.STAGE_LIDAR, F.STAGE_RAW_DEPTH, F.STAGE_RECT_DEPTH, F.STAGE_MAP):
            assert plain.read_stage(stage).tobytes() == swept.read_stage(stage).tobytes()
    plain.close(); swept.close()


def test_the_sweep_is_set_changed_and_cleared_between_frames(pkg):
    """field modes and the azimuth mode in turn (the staged record changes its size with them), no sweep in between,
    other settings of the scan source under a sweep that stays, and the scan source cleared, which takes the sweep along"""
    F = pkg.frontend
    w, h = 96, 64
    seq = TL.SEQS[(w, h)]
    bgr, dep = G.frame(w, h, 72), KM.surface(w, h, 30)
    s = K.setting((1, 7, 1, 0.25), **K.MOUNT)
    gen = TL._generator(pkg, w, h)
    gen.set_lidar(K.to_struct(F, s, max_points=4200))
    k = 0
    for mode, layout in ((S.TIME_F32, (8, 7)), (S.AZIMUTH, (4, 3)), (None, (4, 3)), (S.TIME_U32, (4, 3)), (S.TIME_U32, (8, 3)),
                         (S.AZIMUTH, (4, 3)), (S.TIME_F32, (4, 3))):
        sw = None if mode is None else S.sweep_of(mode, layout, s_ref=0.25 + 0.125 * (k % 3), direction=-1)
        gen.set_lidar_sweep(S.to_struct(F, sw))
        assert gen.lidar_sweep() == S.to_struct(F, sw) and not gen.lidar_motion().any()
        for j in range(2):
            pts = K.scan_clutter(w, h, 3500 + 100 * (k % 5), 90 + k % 2, s, TL._table(F, seq))
            if sw is None:
                TL._lidar_frame(gen, F, bgr, pts, s, seq)
            else:
                _sweep_frame(gen, F, bgr, S.records_of(pts, sw, layout), s, seq, sw, S.TWISTS[("turn", "unit", "shift")[k % 3]])
            k += 1
    assert sw is not None and sw.mode == S.TIME_F32             # (the loop's last sweep is in force)
    s2 = K.setting((2, 3, 1, 0.25), **K.MOUNT)
    gen.set_lidar(K.to_struct(F, s2, max_points=5000))          # other settings and another capacity: the sweep stays
    assert gen.lidar_sweep() == S.to_struct(F, sw)
    pts = K.scan_clutter(w, h, 4900, 95, s2, TL._table(F, seq))
    _sweep_frame(gen, F, bgr, S.records_of(pts, sw), s2, seq, sw, S.TWISTS["turn"])
    gen.set_lidar(None)
    assert gen.lidar_sweep() is None and not gen.lidar_motion().any()
    cloud = gen.create_pointcloud(bgr, dep, seq, F.FEATURES_RGB)
    TL._cloud_equal(gen, F, cloud, bgr, dep, seq, F.FEATURES_RGB)
    gen.set_lidar(K.to_struct(F, s, max_points=4200))
    assert gen.lidar_sweep() is None
    TL._lidar_frame(gen, F, bgr, K.scan_clutter(w, h, 3000, 96, s, TL._table(F, seq)), s, seq)
    gen.close()


def test_the_median_fills_behind_the_moved_plane(pkg):
    F = pkg.frontend
    w, h = 96, 64
    seq, m = TL.SEQS[(w, h)], (1, 2)
    bgr = G.frame(w, h, 72)
    s = K.setting((0, 7, 1, 0.25), **K.MOUNT)
    sw = S.sweep_of(S.TIME_U32)
    rec = S.records_of(K.scan_clutter(w, h, 4097, 52, s, TL._table(F, seq)), sw)
    twist = S.TWISTS["turn"]
    want = S.lidar_sweep(rec, s, TL._table(F, seq), w, h, sw, twist)
    B, mflags, changed, filled = KM.median(want[0], m)
    assert filled >= 100
    gen = TL._generator(pkg, w, h)
    gen.set_depth_median(KM.to_struct(F, m))
    gen.set_lidar(K.to_struct(F, s))
    gen.set_lidar_sweep(S.to_struct(F, sw))
    gen.set_lidar_motion(twist)
    for _ in range(2):
        cloud = gen.create_pointcloud_lidar(bgr, rec, seq, F.FEATURES_RGB)
        TL._planes_equal(gen, F, want, final=B)
        TL._differ(gen.read_stage(F.STAGE_UNFILTERED_DEPTH), want[0], "A of the median stage")
        TL._differ(gen.read_stage(F.STAGE_MEDIAN), mflags, "the median's flags")
        TL._cloud_equal(gen, F, cloud, bgr, B, seq, F.FEATURES_RGB)
    gen.close()


# ---- 3. the refusals ---------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable_and_unchanged(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    w, h = 96, 64
    seq = TL.SEQS[(w, h)]
    bgr, dep = G.frame(w, h, 72), KM.surface(w, h, 30)
    s = K.setting((1, 7, 1, 0.25), **K.MOUNT)
    sw = S.sweep_of(S.TIME_F32, (8, 7))
    good = S.to_struct(F, sw)
    rec = S.records_of(K.scan_clutter(w, h, 4097, 56, s, TL._table(F, seq)), sw, (8, 7))
    twist = S.TWISTS["turn"]
    gen = TL._generator(pkg, w, h)
    plain = gen.create_pointcloud(bgr, dep, seq, F.FEATURES_RGB)
    with pytest.raises(Err):
        gen.set_lidar_sweep(good)                                 # no scan source
    assert b"set_lidar_sweep" in F.lib().cvo_fe_last_error(gen._h)
    with pytest.raises(Err):
        gen.set_lidar_motion(twist)                               # no sweep
    gen.set_lidar_sweep(None)                                     # clearing what is not set is no error
    assert gen.lidar_sweep() is None and _same_cloud(gen.create_pointcloud(bgr, dep, seq, F.FEATURES_RGB), plain)
    gen.set_lidar(K.to_struct(F, s, max_points=4097))
    with pytest.raises(Err):
        gen.set_lidar_motion(twist)                               # a scan source, but no sweep
    for reason, bad in S.bad_sweeps().items():
        with pytest.raises(Err):
            gen.set_lidar_sweep(F.LidarSweep(*bad))
        assert gen.lidar_sweep() is None, reason
    gen.set_lidar_sweep(good)
    cloud, want = _sweep_frame(gen, F, bgr, rec, s, seq, sw, twist)
    for reason, bad in S.bad_sweeps().items():
        with pytest.raises(Err):
            gen.set_lidar_sweep(F.LidarSweep(*bad))
        assert gen.lidar_sweep() == good and np.array_equal(gen.lidar_motion(), np.asarray(twist, f32)), reason
    for reason, bad in S.bad_twists().items():
        with pytest.raises(Err):
            gen.set_lidar_motion(bad)                             # over the caps, or not finite
        assert np.array_equal(gen.lidar_motion(), np.asarray(twist, f32)), reason
    assert b"set_lidar_motion" in F.lib().cvo_fe_last_error(gen._h)
    with pytest.raises(Err):
        gen.submit_lidar(bgr, np.ascontiguousarray(rec[:, :4]), seq)   # a stride of 16 under a time word at 28
    assert b"time_offset" in F.lib().cvo_fe_last_error(gen._h)
    with pytest.raises(Err):
        gen.create_pointcloud_lidar(bgr, np.ascontiguousarray(rec[:, :7]), seq)   # a stride of 28: the word ends at 32
    assert _same_cloud(gen.create_pointcloud_lidar(bgr, rec, seq), cloud)
    gen.submit_lidar(bgr, rec, seq, F.FEATURES_RGB)
    for other in (S.to_struct(F, S.sweep_of(S.AZIMUTH)), good, None):
        with pytest.raises(Err):
            gen.set_lidar_sweep(other)                            # while a frame is in flight, even the sweep in force
    gen.set_lidar_motion(S.TWISTS["shift"])                       # for the frames submitted after the call: not this one
    assert _same_cloud(gen.collect(), cloud) and gen.lidar_sweep() == good
    TL._planes_equal(gen, F, want)
    shifted = S.lidar_sweep(rec, s, TL._table(F, seq), w, h, sw, S.TWISTS["shift"])
    gen.create_pointcloud_lidar(bgr, rec, seq)
    TL._planes_equal(gen, F, shifted)
    gen.set_lidar_sweep(good)                                     # a sweep set: the twist is zero again
    assert not gen.lidar_motion().any()
    gen.close()


# ---- 4. the layers above -----------------------------------------------------------------------------

class _Spy:
    """a generator that notes, at every submit_lidar, the registration's state and the twist in force"""

    def __init__(self, gen, reg):
        self._gen, self._reg, self.seen = gen, reg, []

    def __getattr__(self, name):
        return getattr(self._gen, name)

    def submit_lidar(self, bgr, points, seq, ftype):
        self.seen.append((bool(self._reg.init), self._reg.transform.copy(), self._gen.lidar_motion()))
        self._gen.submit_lidar(bgr, points, seq, ftype)


def _timed_frames(pkg, sw):
    s, frames = TL._lidar_frames(pkg)
    return s, [(name, bgr, S.records_of(pts[:, :3], sw)) for name, bgr, pts in frames]


def test_run_frames_takes_a_callable(pkg):
    """run_frames(lidar_sweep=, lidar_motion=callable) = the generator driven by hand: the twists asked for by name,
    before each frame, and the last plane the restatement's under the last twist"""
    F = pkg.frontend
    sw = S.sweep_of(S.TIME_U32)
    s, frames = _timed_frames(pkg, sw)
    lidar = K.to_struct(F, s, max_points=80000)
    names = [f[0] for f in frames]
    twists = {name: np.asarray(S.TWISTS[t], f32) * f32(0.1) for name, t in zip(names, ("turn", "shift", "zero", "unit"))}
    asked = []

    def motion(name):
        asked.append(name)
        return twists[name]

    reg, gen = pkg.Cvo(), F.PcdGenerator(640, 480)
    spy = _Spy(gen, reg)
    assert F.run_frames(reg, frames, 1, generator=spy, lidar=lidar, lidar_sweep=S.to_struct(F, sw), lidar_motion=motion) == 4
    assert asked == names and gen.lidar_sweep() == S.to_struct(F, sw)
    assert all(np.array_equal(seen[2], twists[name]) for seen, name in zip(spy.seen, names))
    want = S.lidar_sweep(frames[3][2], s, TL._table(F, 1), 640, 480, sw, twists[names[3]])
    assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == want[0].tobytes()
    with pytest.raises(ValueError):
        F.run_frames(reg, frames, 1, generator=gen, lidar_motion="something else")
    reg.close(); gen.close()


def test_run_frames_assumes_a_constant_velocity(pkg):
    """"constant-velocity": zero until a pair is registered, then cvo_fe_lidar_twist of the registration's last
    transform, read back through get_lidar_motion at every submit"""
    F = pkg.frontend
    sw = S.sweep_of(S.AZIMUTH)
    s, frames = _timed_frames(pkg, sw)
    lidar = K.to_struct(F, s, max_points=80000)
    for prefetch in (False, True):
        reg, gen = pkg.Cvo(), F.PcdGenerator(640, 480)
        spy = _Spy(gen, reg)
        assert F.run_frames(reg, frames, 1, generator=spy, lidar=lidar, lidar_sweep=S.to_struct(F, sw),
                            lidar_motion="constant-velocity", sweep_fraction=0.5, prefetch=prefetch) == 4
        assert len(spy.seen) == 4 and not spy.seen[0][0] and not spy.seen[0][2].any()
        moving = 0
        for init, transform, twist in spy.seen:
            want = F.lidar_twist(transform, lidar, 0.5) if init else np.zeros(6, f32)
            assert np.array_equal(twist, want)
            moving += bool(twist.any())
        print("prefetch", prefetch, "frames under a twist", moving, "the last", spy.seen[-1][2])
        assert moving >= 1
        reg.close(); gen.close()


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_the_sweep(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_lidar_sweep / clear_lidar_sweep / set_lidar_motion
    (tests/cpp/cvo_lidar_sweep_demo.cpp): the clouds the C++ object registers and its pose lines equal the Python path's"""
    F = pkg.frontend
    w, h = 640, 480
    sw = S.sweep_of(S.TIME_F32)
    s, frames = _timed_frames(pkg, sw)
    lidar, sweep = K.to_struct(F, s, max_points=80000), S.to_struct(F, sw)
    twists = np.stack([np.asarray(S.TWISTS[t], f32) * f32(0.1) for t in ("turn", "shift", "unit", "turn")])
    carried = [(name, bgr, rec.view(np.uint16).reshape(-1, 128)) for name, bgr, rec in frames]
    got = _demo_lines(tmp_path, "cvo_lidar_sweep_demo", carried, w, h, bytes(lidar) + bytes(sweep) + twists.tobytes(),
                      [mode_name], depth_sizes=True)
    gen = F.PcdGenerator(w, h)
    gen.set_lidar(lidar)
    gen.set_lidar_sweep(sweep)
    bad = ["refused bad sweep", "refused twist over the cap"]

    def prepare(k):
        lines = []
        if k == 2:
            gen.set_lidar_sweep(None)
            gen.set_lidar_sweep(sweep)
            lines = bad + ["refused twist without a sweep"]
        if k == 3:
            gen.set_lidar(None)
            gen.set_lidar(lidar)
            return ["refused twist without a sweep"]
        gen.set_lidar_motion(twists[k])
        return lines

    want, sizes, _ = _device_path_lines(pkg, mode_name, TL._ScanFrames(gen), carried, prepare)
    assert got == ["refused sweep without a scan source", "refused twist without a sweep"] + bad + want
    assert sizes[0] > 100
    gen.close()
