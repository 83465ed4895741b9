"""GPU: frames whose images lie in device memory (cvo_fe_submit_device, cvo_fe_submit_stereo_device; the device-input
contract of include/cvo_frontend.h).  A device frame against the same images submitted from the host, by bits: the cloud,
the info, RECT_BGR and RAW_DEPTH -- dense and pitched, in BGR8, NV12 and a Bayer order, uint16 and float32 depth, a depth
camera's image of its own size, a stereo pair with and without a rig.  Consecutive frames from different tensors (a
captured graph that kept a caller's pointer would show), host and device frames alternating, the caller's tensors left
as they were, the refusals, run_frames and the C++ object above.
The device images are torch tensors (torch.from_numpy(a).to("cuda"); a pitched one is a slice of a wider tensor), handed
over after torch.cuda.synchronize()."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import fe_depth_ref as D
import fe_depthfmt_ref as KD
import fe_gate_ref as G
import fe_stereo_ref as S
import fe_stereo_rig_ref as RG
import fe_unpack_ref as K
from fe_gpu_common import ROOT, _digest, _four_frames, _pose_line_f32, _same_cloud

pytestmark = pytest.mark.gpu

SIZES = ((64, 64), (96, 72))
IDS = ["%dx%d" % s for s in SIZES]


def _torch():
    import torch
    return torch


def _to_device(a, pad=0):
    """(the tensor a frame takes, the whole tensor it is a slice of, the host copy of the whole): `a` with its rows `pad`
    items further apart -- a slice of a wider tensor -- or dense"""
    torch = _torch()
    a = np.ascontiguousarray(a)
    wide = np.full((a.shape[0], a.shape[1] + pad) + a.shape[2:], 0x5A, a.dtype) if pad else a.copy()
    wide[:, :a.shape[1]] = a
    whole = torch.from_numpy(wide).to("cuda")
    view = whole[:, :a.shape[1]] if pad else whole
    torch.cuda.synchronize()
    assert tuple(view.shape) == a.shape
    return view, whole, wide


def _unchanged(*held):
    torch = _torch()
    torch.cuda.synchronize()
    for _, whole, wide in held:
        assert whole.cpu().numpy().tobytes() == wide.tobytes()


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)


def _differ(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s differs at %d places, first at %s" % (what, len(bad), bad[0]))


def _same_frame(dev, host, F, cloud, host_cloud, what, extra=()):
    for stage in (F.STAGE_RECT_BGR, F.STAGE_RAW_DEPTH, F.STAGE_RECT_DEPTH, F.STAGE_MAP) + tuple(extra):
        _differ(dev.read_stage(stage), host.read_stage(stage), "stage %d of %s" % (stage, what))
    assert dev.info() == host.info(), what
    assert _same_cloud(cloud, host_cloud) and len(cloud[0]) >= 20, what


def _frame(w, h, seed=72):
    return G.frame(w, h, seed), G.gate_scene(w, h, seed)


# ---- 1. a device frame is the host frame -------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("fmt", (K.BGR8, K.NV12, K.BAYER_GRBG8), ids=("BGR8", "NV12", "BAYER_GRBG8"))
def test_a_device_frame_equals_the_host_frame(pkg, size, fmt):
    """dense and pitched (NV12 at a pitch of 128, its chroma rows included); uint16 depth dense and at an odd number of
    values per row; each twice: the second frame replays the captured graph"""
    F = pkg.frontend
    w, h = size
    bgr, dep = _frame(w, h)
    packed = bgr if fmt == K.BGR8 else K.pack(bgr, fmt)
    dev, host = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (dev, host):
        g.set_pixel_format(fmt)
    want = host.create_pointcloud(packed, dep, 1, F.FEATURES_RGB)
    pads = (0, 7) if fmt == K.BGR8 else (0, 128 - w) if fmt == K.NV12 else (0, 5)
    for ipad in pads:
        for dpad in (0, 3):
            img, depth = _to_device(packed, ipad), _to_device(dep, dpad)
            for _ in range(2):
                dev.submit_device(img[0], depth[0], 1, F.FEATURES_RGB)
                cloud = dev.collect()
                _same_frame(dev, host, F, cloud, want, "%s pads %d %d" % (K.NAMES[fmt], ipad, dpad),
                            extra=() if fmt == K.BGR8 else (F.STAGE_INPUT_BGR,))
            _unchanged(img, depth)
    dev.close(); host.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_float_depth_from_the_device_is_read_in_place(pkg, size):
    """F32 and F16 depth, dense, pitched and from an address aligned to the value only (a slice that begins one value
    into its row): the conversion reads the caller's image where it lies"""
    F = pkg.frontend
    torch = _torch()
    w, h = size
    bgr, dep = _frame(w, h)
    dev, host = _generator(pkg, w, h), _generator(pkg, w, h)
    img = _to_device(bgr)
    for fmt in KD.FLOATS:
        fl = KD.metres(dep, 4999.0, fmt)
        plane = KD.convert(fl, fmt, 1.0, 5000.0)
        for g in (dev, host):
            g.set_depth_format(fmt)
        want = host.create_pointcloud(bgr, fl, 1, F.FEATURES_RGB)
        _differ(host.read_stage(F.STAGE_RAW_DEPTH), plane, "the host frame's RAW_DEPTH")
        for pad in (0, 1, 3):
            depth = _to_device(fl, pad)
            for _ in range(2):
                dev.submit_device(img[0], depth[0], 1, F.FEATURES_RGB)
                _same_frame(dev, host, F, dev.collect(), want, "%s pad %d" % (KD.NAMES[fmt], pad))
            _unchanged(depth)
        # one value into a wider row: the base is aligned to the value size only
        wide = np.full((h, w + 4), 7.0, fl.dtype)
        wide[:, 1:w + 1] = fl
        whole = torch.from_numpy(wide).to("cuda")
        torch.cuda.synchronize()
        view = whole[:, 1:w + 1]
        assert view.data_ptr() % (4 * fl.dtype.itemsize) != 0
        dev.submit_device(img[0], view, 1, F.FEATURES_RGB)
        _same_frame(dev, host, F, dev.collect(), want, "%s one value in" % KD.NAMES[fmt])
        _unchanged((view, whole, wide))
    _unchanged(img)
    dev.close(); host.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_depth_cameras_image_of_its_own_size(pkg, size):
    F = pkg.frontend
    w, h = size
    rig = D.make_rig(80, 60, (1000.0, 70.0, 70.2, 39.1, 29.4), (-0.12, 0.03, 0.001, -0.002, 0.0), D.K_R, D.K_T)
    raw = D.scene(pkg.data, rig)
    bgr = G.frame(w, h, 72)
    dev, host = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (dev, host):
        g.set_depth_camera(D.to_struct(F, rig))
    want = host.create_pointcloud(bgr, raw, 1, F.FEATURES_RGB)
    for pad in (0, 5):
        img, depth = _to_device(bgr, pad), _to_device(raw, pad)
        for _ in range(2):
            dev.submit_device(img[0], depth[0], 1, F.FEATURES_RGB)
            _same_frame(dev, host, F, dev.collect(), want, "pad %d" % pad)
        _unchanged(img, depth)
    # ... and as float32 metres
    fl = KD.metres(raw, 1000.0)
    for g in (dev, host):
        g.set_depth_format(F.DEPTH_F32)
    want = host.create_pointcloud(bgr, fl, 1, F.FEATURES_RGB)
    img, depth = _to_device(bgr), _to_device(fl, 2)
    dev.submit_device(img[0], depth[0], 1, F.FEATURES_RGB)
    _same_frame(dev, host, F, dev.collect(), want, "float32")
    with pytest.raises(ValueError):
        dev.submit_device(img[0], _to_device(np.zeros((h, w), np.float32))[0], 1, F.FEATURES_RGB)   # (the context's size)
    dev.close(); host.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("rigged", (False, True), ids=("rectified", "rig"))
def test_a_stereo_pair_from_the_device(pkg, size, rigged):
    F = pkg.frontend
    w, h = size
    left, right, _ = S.pair(w, h, 81, box=5.0, back=3.0)
    dev, host = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (dev, host):
        g.set_stereo(S.to_struct(F, S.make_stereo(max_disp=8)))
        if rigged:
            g.set_stereo_rig(RG.to_struct(F, RG.rectify(RG.CALIBS["A"][3], w, h, RG.DEPTH_SCALE)))
    want = host.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    for pad in (0, 3):
        dl, dr = _to_device(left, pad), _to_device(right, pad + 1)
        for _ in range(2):
            dev.submit_stereo_device(dl[0], dr[0], S.SEQ, F.FEATURES_RGB)
            cloud = dev.collect()
            for stage in (F.STAGE_RECT_BGR, F.STAGE_RIGHT_BGR, F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_RAW_DEPTH, F.STAGE_MAP):
                _differ(dev.read_stage(stage), host.read_stage(stage), "stage %d" % stage)
            assert dev.info() == host.info() and _same_cloud(cloud, want)
        _unchanged(dl, dr)
    assert (host.read_stage(F.STAGE_DISPARITY) != 0).any()
    dev.close(); host.close()


# ---- 2. the graph holds no pointer of the caller's ---------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_three_frames_from_three_tensors(pkg, size):
    """three different pictures in three different tensors, all alive at once: each frame is its own host frame"""
    F = pkg.frontend
    w, h = size
    dev, host = _generator(pkg, w, h), _generator(pkg, w, h)
    frames = [_frame(w, h, seed) for seed in (72, 73, 74)]
    held = [(_to_device(bgr, k), _to_device(dep, k)) for k, (bgr, dep) in enumerate(frames)]
    assert len({img[0].data_ptr() for img, _ in held}) == 3 and len({dep[0].data_ptr() for _, dep in held}) == 3
    clouds = []
    for k, ((bgr, dep), (img, depth)) in enumerate(zip(frames, held)):
        want = host.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        dev.submit_device(img[0], depth[0], 1, F.FEATURES_RGB)
        clouds.append(dev.collect())
        _same_frame(dev, host, F, clouds[-1], want, "frame %d" % k)
    assert not _same_cloud(clouds[0], clouds[1]) and not _same_cloud(clouds[1], clouds[2])
    for img, depth in held:
        _unchanged(img, depth)
    dev.close(); host.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_host_and_device_frames_alternate(pkg, size):
    """on one context, with the cloud taken from the host and from the device"""
    F = pkg.frontend
    w, h = size
    dev, host = _generator(pkg, w, h), _generator(pkg, w, h)
    frames = [_frame(w, h, seed) for seed in (72, 73)]
    held = [(_to_device(bgr, 2), _to_device(dep, 1)) for bgr, dep in frames]
    for k in range(8):
        (bgr, dep), (img, depth) = frames[k % 2], held[k % 2]
        on = k % 4 >= 2
        dev.set_device_output(on)
        want = host.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        if k in (0, 3, 4, 7):
            dev.submit_device(img[0], depth[0], 1, F.FEATURES_RGB)
        else:
            dev.submit(bgr, dep, 1, F.FEATURES_RGB)
        if on:
            _, _, n = dev.collect_device()
            assert n == len(want[0])
            for stage in (F.STAGE_RECT_BGR, F.STAGE_RAW_DEPTH, F.STAGE_MAP):
                _differ(dev.read_stage(stage), host.read_stage(stage), "stage %d of frame %d" % (stage, k))
            assert dev.info() == host.info()
        else:
            _same_frame(dev, host, F, dev.collect(), want, "frame %d" % k)
    for img, depth in held:
        _unchanged(img, depth)
    dev.close(); host.close()


# ---- 3. what is refused ------------------------------------------------------------------------------

def test_refusals_enqueue_nothing_and_the_next_frame_is_right(pkg):
    """pinned host memory (the context's own staging images), a pitch below the row, an odd depth pitch: refused with a
    message before anything is enqueued; then an ordinary frame"""
    import ctypes as C
    F = pkg.frontend
    L = F.lib()
    w, h = 64, 64
    bgr, dep = _frame(w, h)
    dev, host = _generator(pkg, w, h), _generator(pkg, w, h)
    want = host.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    img, depth = _to_device(bgr), _to_device(dep)
    pi, pd = img[0].data_ptr(), depth[0].data_ptr()
    h_img, h_dep = dev.host_buffers()
    h_img[:], h_dep[:] = bgr, dep
    pinned_img, pinned_dep = h_img.ctypes.data, h_dep.ctypes.data

    def refused(args, text):
        assert L.cvo_fe_submit_device(dev._h, *args) == -1, args
        assert text in L.cvo_fe_last_error(dev._h).decode(), L.cvo_fe_last_error(dev._h)

    refused((pinned_img, w * 3, pd, w * 2, 1, 1), "colour image is not device memory")
    refused((pi, w * 3, pinned_dep, w * 2, 1, 1), "depth image is not device memory")
    refused((pi, w * 3 - 1, pd, w * 2, 1, 1), "bad argument")
    refused((pi, w * 3, pd, w * 2 - 2, 1, 1), "bad argument")
    refused((pi, w * 3, pd, w * 2 + 1, 1, 1), "not a multiple")
    refused((None, w * 3, pd, w * 2, 1, 1), "bad argument")
    refused((pi, w * 3, pd, w * 2, 1, 7), "bad argument")
    with pytest.raises(ValueError):
        dev.submit_device(bgr, depth[0], 1, F.FEATURES_RGB)           # (a numpy array has no device interface)
    with pytest.raises(ValueError):
        dev.submit_device(img[0], _to_device(dep.astype(np.float16))[0], 1, F.FEATURES_RGB)   # (float16 under U16)
    # nothing is pending; an ordinary frame, host then device, is right
    assert _same_cloud(dev.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want)
    dev.submit_device(img[0], depth[0], 1, F.FEATURES_RGB)
    _same_frame(dev, host, F, dev.collect(), want, "the frame after the refusals")
    # a stereo pair on a context without stereo, and a context with a scan source
    assert L.cvo_fe_submit_stereo_device(dev._h, pi, w * 3, pi, w * 3, 4, 1) == -1
    dev.set_lidar(F.Lidar(max_points=64))
    refused((pi, w * 3, pd, w * 2, 1, 1), "scan source")
    _unchanged(img, depth)
    dev.close(); host.close()


# ---- 4. the layers above -----------------------------------------------------------------------------

def test_run_frames_takes_device_arrays(pkg):
    """run_frames(device_input=True) on the frames as device arrays = run_frames on the host arrays: the same poses"""
    F = pkg.frontend
    frames = _four_frames(pkg, 75)
    held = [(name, _to_device(bgr, 4), _to_device(dep, 2)) for name, bgr, dep in frames]
    on_device = [(name, img[0], depth[0]) for name, img, depth in held]
    poses = []
    for fr, device_input in ((on_device, True), (frames, False)):
        reg, buf = pkg.Cvo(), io.StringIO()
        gen = F.PcdGenerator(640, 480)
        assert F.run_frames(reg, fr, 1, writer=pkg.trajectory.TrajectoryWriter(buf), generator=gen, device_input=device_input) == 4
        _differ(gen.read_stage(F.STAGE_RECT_BGR), frames[3][1], "the last frame's image")
        poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
        reg.close(); gen.close()
    assert poses[1][0] == poses[0][0] and np.array_equal(poses[1][1], poses[0][1]) and poses[1][2] == poses[0][2] > 0
    assert len(poses[0][0].strip().split("\n")) == 4
    for _, img, depth in held:
        _unchanged(img, depth)
    reg = pkg.Cvo()
    with pytest.raises(ValueError, match="device_input"):
        F.run_frames(reg, frames, 1, lidar=F.Lidar(), device_input=True)
    reg.close()


def _demo(tmp_path, frames, w, h, mode_name):
    """builds tests/cpp/cvo_device_input_demo.cpp against the library and the HIP runtime and returns its lines"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "cvo_device_input_demo")
    lib = os.path.join(ROOT, "cvo-rgbd_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), os.path.join(ROOT, "tests", "cpp", "cvo_device_input_demo.cpp"),
                    "-L", lib, "-lcvo_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], check=True, timeout=120)
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<iii", len(frames), w, h))
        for name, bgr, dep in frames:
            fh.write(name.encode().ljust(32, b"\0"))
            fh.write(bgr.tobytes())
            fh.write(dep.tobytes())
    out = subprocess.run([exe, path, mode_name], check=True, capture_output=True, text=True, timeout=120).stdout
    return out.strip().split("\n")


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_device_images(pkg, tmp_path, mode_name):
    """include/cvo.hpp run_cvo_on_device and set_depth_format (tests/cpp/cvo_device_input_demo.cpp): the clouds the C++
    object registers and its pose lines equal those of the Python device path, character for character"""
    F = pkg.frontend
    w, h = 640, 480
    frames = _four_frames(pkg, 75)
    got = _demo(tmp_path, frames, w, h, mode_name)
    acvo = mode_name == "acvo"
    reg = (pkg.Acvo if acvo else pkg.Cvo)()
    gen = F.PcdGenerator(w, h)
    gen.set_device_output(True)
    ftype = F.FEATURES_HSV if acvo else F.FEATURES_RGB
    want, sizes = ["refused a bad depth format"], []
    for k, (name, bgr, dep) in enumerate(frames):
        if k == 2:
            want.append("refused a bad depth format")
            gen.set_depth_format(F.DEPTH_F32, 1.0)
        depth = dep if k < 2 else dep.astype(np.float32) / np.float32(5000.0)
        img, depth = _to_device(bgr, 16), _to_device(depth, 24 if k < 2 else 12)      # (48 bytes, as the demo's)
        gen.submit_device(img[0], depth[0], 1, ftype)
        dp, df, n = gen.collect_device()
        sizes.append(n)
        reg.run_cvo_device(dp, df, n)
        d = reg.ctx.device_cloud(0)
        assert d["points"] == n
        want.append("cloud %s %d %d %d" % (name, n, _digest(d["pos"][:n]), _digest(d["feat"][:n])))
        want.append(_pose_line_f32(name, reg.accum_transform))
    want.append("points_last_frame %d iterations %d" % (sizes[-1], reg.num_iterations))
    reg.close(); gen.close()
    assert got == want
    assert min(sizes) > 100
