"""GPU: the photometric stage of the front end (cvo_fe_set_photometric, cvo_fe_photometric_image; the photometric contract
of include/cvo_frontend.h): k_fe_photo_apply, k_fe_photo_stat and k_fe_photo_gain of csrc/cvo_photo.hip against the
restatement tests/fe_photometric_ref.py -- the image by bytes and the frame's record by value at every size, flag
combination and input of fe_photometric_ref.cases() -- and frames of every kind: the corrected input image by bytes
against the restatement, and every later stage, the info and the cloud, by bytes and bits, against a second context
without the stage that was fed the restatement's image.  Gains that change under a captured graph, the lock of AUTO over
a sequence, the setting alternating with off with and without graphs, the refusals with their sentences, the memory,
run_frames and the C++ objects above.  Which errors of kernels of this shape these inputs would show is asserted in
tests/test_fe_photometric_cpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_binning_ref as B
import fe_gate_ref as G
import fe_lidar_ref as KL
import fe_photometric_ref as P
import fe_rectify_ref as R
import fe_stereo_ref as S
import fe_unpack_ref as K
from fe_gpu_common import ROOT, _demo_lines, _device_path_lines, _four_frames, _same_cloud

pytestmark = pytest.mark.gpu

SIZES = ((64, 64), (96, 64))
IDS = ["%dx%d" % s for s in SIZES]
RULE = b"flags a non-empty OR of CVO_FE_PHOTO_*"


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)


def _differ(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s differs at %d places, first at %s: %s against %s"
                             % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _later_stages(F):
    return (F.STAGE_RECT_BGR, F.STAGE_GRAY, F.STAGE_RECT_DEPTH, F.STAGE_RAW_DEPTH, F.STAGE_UNGATED_DEPTH, F.STAGE_HSV,
            F.STAGE_MAP, F.STAGE_AG0, F.STAGE_AG1, F.STAGE_AG2, F.STAGE_THS, F.STAGE_DX0, F.STAGE_DY0)


def _same_frame(gen, plain, F, cloud, plain_cloud, what, extra=()):
    """every later stage by bytes, the info, and the cloud by bits: the frame of the context without the stage"""
    for stage in _later_stages(F) + tuple(extra):
        _differ(gen.read_stage(stage), plain.read_stage(stage), "stage %d of %s" % (stage, what))
    assert gen.info() == plain.info(), what
    print("%s: %d points" % (what, len(cloud[0])))
    assert _same_cloud(cloud, plain_cloud) and len(cloud[0]) >= 20, what


def _setup(w, h, iw=None, ih=None):
    """the setting of the frame tests: both tables, and the caller's gains at 64 x 64, AUTO per channel with a target at
    96 x 64.  The vignette is of the input size iw x ih."""
    iw, ih = iw or w, ih or h
    if w == 64:
        return P.setting(P.GAIN | P.RESPONSE | P.VIGNETTE), P.response(), P.vignette(iw, ih), (5000, 4096, 3300)
    return (P.setting(P.AUTO | P.RESPONSE | P.VIGNETTE, per_channel=1, target=P.TARGET, min_count=16), P.response(),
            P.vignette(iw, ih), None)


def _set(F, gen, setup):
    s, resp, vig, gains = setup
    gen.set_photometric(P.to_struct(F, s), resp, vig)
    if gains is not None:
        gen.set_photometric_gain(np.array(gains, np.float64) / 4096.0)
    assert gen.photometric() == P.to_struct(F, s)


def _want(setup, img, right=None):
    s, resp, vig, gains = setup
    return P.frame(img, s, resp, vig, gains, right=right)


def _record(gen, want):
    assert P.record_of(gen.photometric_frame()) == want


# ---- 1. the stand-alone entry ------------------------------------------------------------------------

@pytest.mark.parametrize("size", P.SIZES, ids=["%dx%d" % s for s in P.SIZES])
def test_photometric_image_by_bytes(pkg, size):
    """every flag combination, per_channel 0 and 1, and every input of the size: the image by bytes, the record by value;
    the source is left as it is (photometric_image checks it)"""
    F = pkg.frontend
    n = 0
    for case in P.cases((size,)):
        name, w, h, s, resp, vig, gains, kind = case
        img = P.case_image(case)
        want, rec = P.case_frame(case)
        got, grec = F.photometric_image(img, P.to_struct(F, s), resp, vig, gains)
        _differ(got, want, "%s %s" % (name, kind))
        assert P.record_of(grec) == rec, (name, kind, P.record_of(grec), rec)
        n += 1
    assert n == 3 + 4 * 2 + 16 * 5


def test_a_size_past_the_grid_of_the_statistic(pkg):
    """k_fe_photo_stat runs at most 2048 blocks of 256 threads, four pixels a thread and round: 2049 x 1025 is the smallest
    odd size at which some threads go round twice, and its block sums pass 32 bits where the whole image counts"""
    F = pkg.frontend
    w, h = 2049, 1025
    assert (w * h + 3) // 4 > 2048 * 256 and (w * h) % 4 == 1
    rng = np.random.RandomState(11)
    img = rng.randint(8, 248, (h, w, 3)).astype(np.uint8)
    resp, vig = P.response("max"), np.full((h, w), 65535, np.uint16)
    for s, r, v in ((P.setting(P.AUTO | P.RESPONSE | P.VIGNETTE, per_channel=1, target=(65535,) * 3, gain_min=1), resp, vig),
                    (P.setting(P.AUTO, per_channel=0, target=P.TARGET), None, None)):
        want, rec, _ = P.frame(img, s, r, v)
        got, grec = F.photometric_image(img, P.to_struct(F, s), r, v)
        _differ(got, want, "2049x1025 flags %d" % s[0])
        assert P.record_of(grec) == rec and rec["count"] == w * h and rec["flags"] == 0
        if r is not None:
            assert min(rec["sum"]) == w * h * ((65535 * 65535) >> 12) > 2 ** 40


def test_the_entry_takes_a_row_stride(pkg):
    """rows further apart than their bytes, row + 5 (the vignette's: row + 5 values): what lies between them is not read
    into the image, and stays"""
    F = pkg.frontend
    for w, h in ((13, 7), (66, 18), (130, 34)):
        for flags in (P.GAIN | P.RESPONSE | P.VIGNETTE, P.AUTO | P.VIGNETTE):
            s = P.setting(flags, per_channel=1, target=P.TARGET)
            resp = P.response() if flags & P.RESPONSE else None
            img = P.image(w, h, "random")
            want, rec, _ = P.frame(img, s, resp, P.vignette(w, h), (5851, 4096, 3000))
            got, grec = F.photometric_image(img, P.to_struct(F, s), resp, P.vignette(w, h), (5851, 4096, 3000), stride=w * 3 + 5,
                                            vignette_stride=w + 5)
            _differ(got, want, "%dx%d flags %d" % (w, h, flags))
            assert P.record_of(grec) == rec


# ---- 2. frames ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_depth_frame(pkg, size):
    F = pkg.frontend
    w, h = size
    setup = _setup(w, h)
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    want, rec, _ = _want(setup, bgr)
    assert not np.array_equal(want, bgr)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    assert gen.photometric() is None
    _set(F, gen, setup)
    for k in range(2):                                        # (the second frame replays the captured graph)
        ftype = F.FEATURES_HSV if k else F.FEATURES_RGB
        cloud = gen.create_pointcloud(bgr, dep, 1, ftype)
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), want, "INPUT_BGR")
        _record(gen, rec)
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud(want, dep, 1, ftype), "depth frame")
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_stereo_frame(pkg, size):
    """both images through the same tables and the same G; the statistic is the left image's"""
    F = pkg.frontend
    w, h = size
    setup = _setup(w, h)
    st = S.make_stereo(max_disp=32)
    left, right, _ = S.pair(w, h, 82)
    right = P.darkened(right, 0.8)
    wl, rec, _, wr = _want(setup, left, right)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    plain.set_stereo(S.to_struct(F, st))
    if w == 64:                                               # (the stage first, stereo behind it ...)
        _set(F, gen, setup)
        gen.set_stereo(S.to_struct(F, st))
    else:                                                     # (... and the other way round)
        gen.set_stereo(S.to_struct(F, st))
        _set(F, gen, setup)
    assert gen.photometric() == P.to_struct(F, setup[0]) and gen.stereo() == S.to_struct(F, st)
    for _ in range(2):
        cloud = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), wl, "INPUT_BGR")
        _differ(gen.read_stage(F.STAGE_INPUT_RIGHT_BGR), wr, "INPUT_RIGHT_BGR")
        _record(gen, rec)
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud_stereo(wl, wr, S.SEQ, F.FEATURES_RGB), "stereo",
                    extra=(F.STAGE_RIGHT_BGR, F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_RIGHT_GRAY))
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_lidar_frame(pkg, size):
    F = pkg.frontend
    w, h = size
    setup = _setup(w, h)
    seq = 4
    cam = tuple(F.camera(seq).values())
    s = KL.setting((1, 7, 1, 0.25), **KL.MOUNT)
    points = KL.scan_clutter(w, h, 4097, 52, s, cam)
    bgr, _ = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    want, rec, _ = _want(setup, bgr)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    _set(F, gen, setup)
    gen.set_lidar(KL.to_struct(F, s)); plain.set_lidar(KL.to_struct(F, s))
    assert gen.photometric() == P.to_struct(F, setup[0])
    for _ in range(2):
        cloud = gen.create_pointcloud_lidar(bgr, points, seq, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), want, "INPUT_BGR")
        _record(gen, rec)
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud_lidar(want, points, seq, F.FEATURES_RGB), "lidar",
                    extra=(F.STAGE_LIDAR_DEPTH, F.STAGE_LIDAR))
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_frame_under_a_pixel_format(pkg, size):
    """Bayer RGGB and NV12: the stage runs behind the unpack, on what it wrote; the format before the stage for the mosaic,
    behind it for NV12"""
    F = pkg.frontend
    w, h = size
    setup = _setup(w, h)
    _, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for fmt in (K.BAYER_RGGB8, K.NV12):
        packed = K.pack(G.frame(w, h, 72), fmt)
        want, rec, _ = _want(setup, K.unpack(packed, fmt, w, h))
        gen.set_photometric(None)
        gen.set_pixel_format(K.BGR8)
        if fmt == K.NV12:
            _set(F, gen, setup)
            gen.set_pixel_format(fmt)
        else:
            gen.set_pixel_format(fmt)
            _set(F, gen, setup)
        assert gen.pixel_format() == fmt and gen.photometric() == P.to_struct(F, setup[0])
        for _ in range(2):
            cloud = gen.create_pointcloud(packed, dep, 1, F.FEATURES_RGB)
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), want, "INPUT_BGR under " + K.NAMES[fmt])
            _record(gen, rec)
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(want, dep, 1, F.FEATURES_RGB), K.NAMES[fmt])
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_frame_under_binning(pkg, size):
    """f = 2 and a vignette of the input size: the stage corrects the input-size image, the bin averages what it wrote"""
    F = pkg.frontend
    w, h = size
    f = 2
    setup = _setup(w, h, f * w, f * h)
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=f * w, height=f * h, seed=72, texture=1.0, holes=0.02)
    want, rec, _ = _want(setup, bgr)
    bbgr, bdep = B.bin_colour(want, f), B.bin_depth(dep, f, 1)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    gen.set_input_binning(F.Binning(f, 1))
    _set(F, gen, setup)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_FULL_BGR), want, "FULL_BGR")
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), bbgr, "INPUT_BGR")
        _record(gen, rec)
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB), "binning")
    # the input size does not change under a vignette, and says which size it has
    for other in (None, F.Binning(3, 1)):
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_input_binning(other)
        msg = F.lib().cvo_fe_last_error(gen._h)
        assert msg.startswith(b"set_input_binning: a vignette of %d x %d is set" % (f * w, f * h)), msg
        assert (b"%d x %d" % ((w, h) if other is None else (3 * w, 3 * h))) in msg
    gen.set_input_binning(F.Binning(f, 4))                     # (depth_min alone: the size stays)
    assert gen.photometric() == P.to_struct(F, setup[0])
    gen.set_photometric(None)
    gen.set_input_binning(None)
    gen.close(); plain.close()


def test_a_distorting_model(pkg):
    """model A (96 x 64): k_fe_rectify resamples what the stage wrote"""
    F = pkg.frontend
    w, h, model = R.SMALL["A"]
    setup = _setup(w, h)
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    want, rec, _ = _want(setup, bgr)
    qu, qv = R.rectify_map(model, w, h)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    _set(F, gen, setup)
    gen.set_camera(F.CameraModel(*model)); plain.set_camera(F.CameraModel(*model))
    assert gen.photometric() == P.to_struct(F, setup[0])
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), want, "INPUT_BGR")
        _differ(gen.read_stage(F.STAGE_RECT_BGR), R.remap_colour(want, qu, qv), "RECT_BGR")
        _record(gen, rec)
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud(want, dep, 1, F.FEATURES_RGB), "model A")
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_device_input(pkg, size):
    """the images in device memory, dense and as slices of wider tensors; the caller's tensors are left as they are"""
    import torch
    F = pkg.frontend
    w, h = size
    setup = _setup(w, h)
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    want, rec, _ = _want(setup, bgr)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    _set(F, gen, setup)
    ref = plain.create_pointcloud(want, dep, 1, F.FEATURES_RGB)
    for pad in (0, 3):
        wide_i = np.full((h, w + pad, 3), 0x5A, np.uint8)
        wide_i[:, :w] = bgr
        wide_d = np.full((h, w + pad), 0x5A5A, np.uint16)
        wide_d[:, :w] = dep
        ti, td = torch.from_numpy(wide_i).to("cuda"), torch.from_numpy(wide_d).to("cuda")
        torch.cuda.synchronize()
        for _ in range(2):
            gen.submit_device(ti[:, :w], td[:, :w], 1, F.FEATURES_RGB)
            cloud = gen.collect()
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), want, "INPUT_BGR")
            _record(gen, rec)
            _same_frame(gen, plain, F, cloud, ref, "device input pad %d" % pad)
        torch.cuda.synchronize()
        assert ti.cpu().numpy().tobytes() == wide_i.tobytes() and td.cpu().numpy().tobytes() == wide_d.tobytes()
    gen.close(); plain.close()


# ---- 3. the frame's header and the lock --------------------------------------------------------------

def test_six_frames_under_a_captured_graph_with_gains_that_change(pkg):
    """one graph, six gains: each frame is corrected under its own, and the record says so"""
    F = pkg.frontend
    assert os.environ.get("CVO_FE_NO_GRAPH") is None
    w, h = 96, 64
    s = P.setting(P.GAIN | P.VIGNETTE, gain_min=2000, gain_max=9000)
    vig = P.vignette(w, h)
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    gen.set_photometric(P.to_struct(F, s), None, vig)
    gains = ((1.0, 1.0, 1.0), (1.25, 1.0, 0.8), (0.7, 0.7, 0.7), (1.0 / 0.7,) * 3, (0.0625, 15.99, 1.0), (1.1, 1.2, 1.3))
    seen = set()
    for k, g in enumerate(gains):
        if k:                                                 # (frame 0: the gains a setter leaves, 1)
            gen.set_photometric_gain(g)
        q = tuple(P.gain_q12(v) for v in g)
        want, rec, _ = P.frame(bgr, s, None, vig, q)
        cloud = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), want, "INPUT_BGR of frame %d" % k)
        _record(gen, rec)
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud(want, dep, 1, F.FEATURES_RGB), "frame %d" % k)
        seen.add(want.tobytes())
    assert len(seen) == 6 and rec["gain"] == (4506, 4915, 5325)
    assert P.record_of(gen.photometric_frame())["gain"] != (4096,) * 3
    for bad in ((np.nan, 1, 1), (1, np.inf, 1), (0.06, 1, 1), (1, 1, 16.0), (-1.0, 1, 1)):
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_photometric_gain(bad)
        assert b"set_photometric_gain: three finite gains in [1/16, 15.99]" == F.lib().cvo_fe_last_error(gen._h)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), cloud)   # (the gains held)
    gen.close(); plain.close()


@pytest.mark.parametrize("per_channel", (0, 1))
def test_the_lock_of_auto_over_a_sequence(pkg, per_channel):
    """the third frame darkened, the fifth without a counted pixel (FALLBACK, the lock untouched), then rearm"""
    F = pkg.frontend
    w, h = 64, 64
    s = P.setting(P.AUTO, per_channel=per_channel, min_count=100)
    frames = P.auto_sequence(w, h)
    want = P.run_sequence(frames, s, rearm_at=(5,))
    _, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    gen = _generator(pkg, w, h)
    gen.set_photometric(P.to_struct(F, s))
    for k, img in enumerate(frames):
        if k == 5:
            gen.photometric_rearm()
        gen.create_pointcloud(img, dep, 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), want[k][0], "INPUT_BGR of frame %d" % k)
        assert P.record_of(gen.photometric_frame()) == want[k][1], k
    assert [r["flags"] for _, r in want] == [P.LOCKED, 0, 0, 0, P.FALLBACK, P.LOCKED]
    assert np.abs(want[2][0].astype(int) - frames[0].astype(int)).max() <= 2     # the darkened frame came back
    gen.set_photometric(P.to_struct(F, s))                    # the setter opens the lock as well
    gen.create_pointcloud(frames[2], dep, 1, F.FEATURES_RGB)
    rec = P.record_of(gen.photometric_frame())
    assert rec["flags"] == P.LOCKED and rec == P.frame(frames[2], s)[1]
    gen.close()


# ---- 4. the context ----------------------------------------------------------------------------------

def _alternating(pkg):
    """the setting and off alternating on one context, two pictures alternating: off frames are by bits what a fresh
    context gives, on frames what the restatement's image gives.  A graph captured under another setting launched again
    would give that frame's."""
    F = pkg.frontend
    w, h = 96, 64
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    setups = (_setup(64, 64, w, h), None, _setup(w, h), (P.setting(P.RESPONSE), P.response(), None, None), None,
              (P.setting(P.AUTO), None, None, None), _setup(64, 64, w, h), None)
    sizes = []
    for k, setup in enumerate(setups):
        if setup is None:
            gen.set_photometric(None)
            assert gen.photometric() is None
        else:
            _set(F, gen, setup)
        for j in range(2):
            ftype = F.FEATURES_HSV if (k + j) % 3 == 0 else F.FEATURES_RGB
            bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72 + j, texture=1.0)
            if setup is None:
                want = bgr
            elif setup[0][0] & P.AUTO and not any(setup[0][5]):
                want = P.run_sequence([pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72 + i, texture=1.0)[0]
                                       for i in range(j + 1)], setup[0])[j][0]
            else:
                want = _want(setup, bgr)[0]
            cloud = gen.create_pointcloud(bgr, dep, 1, ftype)
            if setup is not None:
                _differ(gen.read_stage(F.STAGE_INPUT_BGR), want, "INPUT_BGR of frame %d.%d" % (k, j))
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(want, dep, 1, ftype), "frame %d.%d" % (k, j))
            sizes.append(len(cloud[0]))
    gen.close(); plain.close()
    return sizes


def test_the_setting_alternates_with_off_on_one_context(pkg):
    assert os.environ.get("CVO_FE_NO_GRAPH") is None
    assert len(_alternating(pkg)) == 16


def test_the_setting_alternates_without_captured_graphs():
    """... and in a session that has CVO_FE_NO_GRAPH in its environment from the start (the library reads it once)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import __graft_entry__ as ge, test_gpu_fe_photometric as T\n"
            "print('sizes', T._alternating(ge.load_package()))\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, CVO_FE_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "sizes [" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_refusals_carry_their_sentence_and_leave_the_context_unchanged(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    L = F.lib()
    message = lambda gen: L.cvo_fe_last_error(gen._h)
    w, h = 96, 64
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    setup = _setup(64, 64, w, h)
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    want = plain.create_pointcloud(_want(setup, bgr)[0], dep, 1, F.FEATURES_RGB)
    _set(F, gen, setup)
    good = P.to_struct(F, setup[0])
    resp, vig = setup[1], setup[2]
    bad_settings = [P.setting(P.GAIN | P.AUTO | 3), P.setting(16 | 3), P.setting(7, lo=9, hi=8), P.setting(7, hi=256),
                    P.setting(7, lo=-1), P.setting(7, min_count=0), P.setting(7, per_channel=2), P.setting(7, target=(65536, 0, 0)),
                    P.setting(7, gain_min=0), P.setting(7, gain_min=5000, gain_max=4999), P.setting(7, gain_max=65536),
                    P.setting(7, pad=1)]
    for s in bad_settings:
        with pytest.raises(Err):
            gen.set_photometric(P.to_struct(F, s), resp, vig)
        assert message(gen).startswith(b"set_photometric: " + RULE) and gen.photometric() == good, s
        assert not P.check(s, True, True)
    # a table without its flag, a flag without its table
    for s, r, v in ((P.setting(P.GAIN | P.RESPONSE), resp, vig), (P.setting(P.GAIN | P.RESPONSE), None, None),
                    (P.setting(P.GAIN | P.VIGNETTE), None, None), (P.setting(P.GAIN), resp, None), (P.setting(0), resp, None)):
        with pytest.raises(Err):
            gen.set_photometric(P.to_struct(F, s), r, v)
        assert message(gen).startswith(b"set_photometric: " + RULE) and gen.photometric() == good
    # a vignette of another size (the Python object's check), and rows too close (the library's, naming the size)
    with pytest.raises(ValueError):
        gen.set_photometric(good, resp, P.vignette(h, w))
    u16p = C.POINTER(C.c_uint16)
    for stride in (w * 2 - 2, w * 2 + 1):
        assert L.cvo_fe_set_photometric(gen._h, C.byref(good), resp.ctypes.data_as(u16p), vig.ctypes.data_as(u16p), stride) == -1
        assert message(gen).startswith(b"set_photometric: a vignette of 96 x 64 uint16"), message(gen)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want)
    # a frame in flight: refused, even "off"; the gains are a frame's own and may be set
    gen.submit(bgr, dep, 1, F.FEATURES_RGB)
    for other in (good, None):
        with pytest.raises(Err):
            gen.set_photometric(other, *((resp, vig) if other is not None else ()))
        assert b"set_photometric: a frame is in flight" == message(gen)
    assert _same_cloud(gen.collect(), want) and gen.photometric() == good
    # the calls that need another setting
    with pytest.raises(Err):
        gen.photometric_rearm()
    assert b"photometric_rearm: the stage is not set with CVO_FE_PHOTO_AUTO" in message(gen)
    gen.set_photometric(P.to_struct(F, P.setting(P.AUTO)))
    with pytest.raises(Err):
        gen.set_photometric_gain(1.0)
    assert b"set_photometric_gain: the stage is not set with CVO_FE_PHOTO_GAIN" in message(gen)
    gen.set_photometric(P.to_struct(F, P.setting(0)))         # (flags 0 and no tables: off)
    assert gen.photometric() is None
    for call in (gen.photometric_rearm, gen.photometric_frame, lambda: gen.set_photometric_gain(1.0)):
        with pytest.raises(Err):
            call()
    with pytest.raises(Err):
        gen.read_stage(F.STAGE_INPUT_BGR)                      # (as before the stage: no such plane on a BGR8 context)
    assert L.cvo_fe_get_photometric(gen._h, None, None) == -1 and L.cvo_fe_set_photometric(None, C.byref(good), None, None, 0) == -1
    assert L.cvo_fe_set_photometric_gain(None, None) == -1 and L.cvo_fe_photometric_rearm(None) == -1
    gen.close(); plain.close()
    # the stand-alone entry
    img, out = np.zeros((2, 4, 3), np.uint8), np.zeros((2, 4, 3), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    i, o, s = img.ctypes.data_as(u8p), out.ctypes.data_as(u8p), C.byref(F.Photometric(P.GAIN))
    call = L.cvo_fe_photometric_image
    assert call(0, None, 4, 2, 12, s, None, None, 0, None, o, None) == -1 and call(0, i, 4, 2, 12, s, None, None, 0, None, None, None) == -1
    assert call(0, i, 4, 2, 11, s, None, None, 0, None, o, None) == -1 and call(0, i, 0, 2, 12, s, None, None, 0, None, o, None) == -1
    assert call(0, i, 8193, 1, 8193 * 3, s, None, None, 0, None, o, None) == -1 and call(0, i, 4, 2, 12, None, None, None, 0, None, o, None) == -1
    assert call(0, i, 4, 2, 12, C.byref(F.Photometric(P.GAIN | P.AUTO)), None, None, 0, None, o, None) == -1
    assert call(0, i, 4, 2, 12, s, None, None, 0, None, o, None) == 0 and not out.any()


def test_the_stage_takes_memory_only_once_set_and_gives_it_back(pkg):
    """On a context of 4096 x 2048 the vignette is 16 MiB on the device, twice the 8 MiB a reading of the free device
    memory resolves.  Refused settings leave it where it was, and at off it is that of a context that never made the call."""
    import torch
    F = pkg.frontend
    MiB = 1024 * 1024

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    w, h = 4096, 2048
    gen = F.PcdGenerator(w, h)
    vig = np.full((h, w), 5000, np.uint16)
    free0 = free()
    with pytest.raises(pkg.capi.CvoHipError):
        gen.set_photometric(F.Photometric(P.VIGNETTE | P.GAIN | P.AUTO), None, vig)
    gen.set_photometric(None)
    free1 = free()
    assert abs(free0 - free1) < 8 * MiB, "refused calls took %d bytes" % (free0 - free1)
    gen.set_photometric(F.Photometric(P.VIGNETTE), None, vig)
    free2 = free()
    assert free1 - free2 >= 16 * MiB - 8 * MiB, "the setting took only %d bytes" % (free1 - free2)
    gen.set_photometric(F.Photometric(P.VIGNETTE | P.AUTO), None, vig)     # (made again: the old tables go)
    assert abs(free() - free2) < 8 * MiB
    gen.set_photometric(None)
    free3 = free()
    assert abs(free3 - free0) < 8 * MiB, "at off the free memory is %d bytes from where it was" % (free0 - free3)
    gen.close()


# ---- 5. the caller-side paths ------------------------------------------------------------------------

def test_run_frames_takes_the_exposures(pkg):
    """run_frames(exposures=): frame i runs under exposures[0] / exposures[i] on all channels"""
    F = pkg.frontend
    frames = _four_frames(pkg, 75)
    exposures = (0.010, 0.014, 0.007, 0.010)
    seen = []

    class Spy(F.PcdGenerator):
        def collect_device(self):
            out = super().collect_device()
            seen.append((P.record_of(self.photometric_frame()), self.read_stage(F.STAGE_INPUT_BGR)))
            return out

    gen = Spy(640, 480)
    reg = pkg.Cvo()
    assert F.run_frames(reg, frames, 1, generator=gen, exposures=exposures) == 4
    assert gen.photometric() == F.Photometric(F.PHOTO_GAIN)
    for k, (rec, img) in enumerate(seen):
        q = P.gain_q12(np.float32(exposures[0] / exposures[k]))
        assert rec["gain"] == (q, q, q), k
        _differ(img, P.frame(frames[k][1], P.setting(P.GAIN), gains_q12=(q, q, q))[0], "INPUT_BGR of frame %d" % k)
    assert [r["gain"][0] for r, _ in seen] == [4096, 2926, 5851, 4096]
    with pytest.raises(ValueError):
        F.run_frames(reg, frames[:1], 1, generator=gen, photometric=F.Photometric(F.PHOTO_AUTO), exposures=exposures)
    reg.close(); gen.close()


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_the_stage(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_photometric (tests/cpp/cvo_photometric_demo.cpp): the clouds the C++ object
    registers and its pose lines equal those of the Python path without the stage on the restatement's images"""
    F = pkg.frontend
    w, h = 320, 240
    frames = [(name, np.ascontiguousarray(bgr[::2, ::2]), np.ascontiguousarray(dep[::2, ::2])) for name, bgr, dep in _four_frames(pkg, 75)]
    s = P.setting(P.GAIN | P.RESPONSE | P.VIGNETTE)
    resp, vig = P.response(), P.vignette(w, h)
    gains = np.array([[1.0, 1.0, 1.0], [1.2, 1.1, 0.9], [1.0, 1.0, 1.0], [0.8, 0.85, 0.9]], np.float32)
    corrected = [(name, bgr if k == 2 else P.frame(bgr, s, resp, vig, tuple(P.gain_q12(g) for g in gains[k]))[0], dep)
                 for k, (name, bgr, dep) in enumerate(frames)]
    settings = bytes(P.to_struct(F, s)) + resp.tobytes() + vig.tobytes() + gains.tobytes()
    got = _demo_lines(tmp_path, "cvo_photometric_demo", frames, w, h, settings=settings, args=(mode_name,))
    gen = F.PcdGenerator(w, h)
    want, sizes, _ = _device_path_lines(pkg, mode_name, gen, corrected, lambda k: ["refused a bad photometric"] if k == 3 else [])
    assert got == ["refused a bad photometric"] + want
    assert min(sizes) > 100
    gen.close()
