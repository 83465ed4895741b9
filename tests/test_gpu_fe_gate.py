"""GPU: the depth gate of the front end (cvo_fe_set_depth_gate, cvo_fe_set_mask, include/cvo_frontend.h):
k_fe_depth_gate against the numpy restatement of the gate contract (tests/fe_gate_ref.py) by bytes and,
downstream of it, the CPU restatement of the front end (oracle/frontend_oracle.c) applied to the
reference-gated depth: every cloud bit for bit.  The stages in front of the gate (rectification,
registration), the captured graphs across changes of gate and mask, the unchanged path without either,
the refusals, and the Python and C++ layers above.  What the shared (scene, gate) cases reach is asserted
in tests/test_fe_gate_cpu.py."""
import ctypes as C
import io

import numpy as np
import pytest

import fe_depth_ref as D
import fe_gate_ref as G
import fe_rectify_ref as R
from conftest import low_texture_frame
from fe_gpu_common import _demo_lines, _device_path_lines, _four_frames, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
_REF = {}


def _ref(key, make):
    """A reference result, computed once per key and left unchanged."""
    if key not in _REF:
        out = make()
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _case(name, w, h, seed):
    """(gate, U, mask, reference depth, reference flags) of a shared case"""
    gate, U, mask = G.case_inputs(name, w, h, seed)
    dep, flags = _ref((name, w, h, seed), lambda: G.gate(U, gate, G.SCALE, mask))
    return gate, U, mask, dep, flags


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=max(200, w * h // 100))


def _planes_equal(gen, F, U, dep, flags):
    assert gen.read_stage(F.STAGE_UNGATED_DEPTH).tobytes() == U.tobytes(), "the plane the gate read"
    assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == dep.tobytes(), "gated depth"
    assert gen.read_stage(F.STAGE_GATE).tobytes() == flags.tobytes(), "flags"


# ---- 1. the gated plane and the flags by bytes -------------------------------------------------

@pytest.mark.parametrize("size", G.SIZES, ids=["%dx%d" % s for s in G.SIZES])
@pytest.mark.parametrize("name", list(G.CASES))
def test_gated_depth_and_flags_by_bytes(pkg, name, size):
    """Every shared case at 64 x 64 (the smallest image), 96 x 64 and 127 x 193 (a width that is no multiple of four:
    the pixel-by-pixel path; neither side a multiple of the tile), three seeds.  The case "seams" puts its steps
    on the seams of the kernel's tile of 64 x 16 pixels (x = 64, y = 16, 32, 48, ...) and on all four borders."""
    F = pkg.frontend
    w, h = size
    gen = _generator(pkg, w, h)
    for seed in G.SEEDS:
        gate, U, mask, dep, flags = _case(name, w, h, seed)
        bgr = G.frame(w, h, seed)
        gen.set_depth_gate(None)
        gen.set_mask(None)
        gen.create_pointcloud(bgr, U, 1, F.FEATURES_RGB)
        before = gen.read_stage(F.STAGE_RECT_DEPTH)
        assert np.array_equal(before, U)
        gen.set_depth_gate(G.to_struct(F, gate))
        gen.set_mask(mask)
        assert gen.depth_gate() == G.to_struct(F, gate)
        gen.create_pointcloud(bgr, U, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, before, dep, flags)
        assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), U)
        assert np.array_equal(gen.read_stage(F.STAGE_RECT_BGR), bgr)
        assert flags.any() and np.count_nonzero(dep) >= np.count_nonzero(U) // 4
    gen.close()


def test_range_edge_at_scale_5000(pkg):
    """the table's row 1 counts 5000 units per metre: under min_range = 0.8f a pixel of 4000 is kept, 3999 is dropped"""
    F = pkg.frontend
    w, h = 64, 64
    U = np.full((h, w), 4000, np.uint16)
    U[::2, 1::2] = 3999
    U[5, 5] = 20000; U[5, 7] = 20001
    gen = _generator(pkg, w, h)
    gen.set_depth_gate(F.DepthGate(0.8, 4.0))
    gen.create_pointcloud(G.frame(w, h, 72), U, 1, F.FEATURES_RGB)
    want = np.where((U == 3999) | (U == 20001), 0, U).astype(np.uint16)
    assert np.array_equal(gen.read_stage(F.STAGE_RECT_DEPTH), want)
    assert np.array_equal(gen.read_stage(F.STAGE_GATE), np.where(want == 0, G.RANGE, 0))
    assert np.array_equal(want, G.gate(U, G.make_gate(0.8, 4.0), 5000.0)[0])
    gen.close()


# ---- 2. the stages in front of the gate --------------------------------------------------------

@pytest.mark.parametrize("model_name", ["A", "C"])
def test_the_mask_follows_a_distorting_model(pkg, model_name):
    """k_fe_rectify writes the plane the gate reads, and the mask goes through the same map (C: an odd width)"""
    F = pkg.frontend
    w, h, model = R.SMALL[model_name]
    gate = dict(G.FULL, grow=1)
    U0 = G.gate_scene(w, h, 72)
    bgr = G.frame(w, h, 72)
    mask = G.mask_scene(w, h, 72)
    qu, qv = R.rectify_map(model, w, h)
    U = R.remap_depth(U0, qu, qv)
    dep, flags = G.gate(U, gate, model[0], mask, qu, qv)
    plain = G.gate(U, gate, model[0], mask)[1]
    assert not np.array_equal(flags, plain)
    gen = _generator(pkg, w, h)
    gen.set_camera(F.CameraModel(*model))
    gen.set_depth_gate(G.to_struct(F, gate))
    gen.set_mask(mask)
    for _ in range(2):
        gen.create_pointcloud(bgr, U0, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, U, dep, flags)
        assert np.array_equal(gen.read_stage(F.STAGE_RECT_BGR), R.remap_colour(bgr, qu, qv))
        assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), U0)
    # the model cleared: the mask is taken as it is, the depth as uploaded
    gen.set_camera(None)
    gen.create_pointcloud(bgr, U0, 1, F.FEATURES_RGB)
    dep1, flags1 = G.gate(U0, gate, G.SCALE, mask)
    _planes_equal(gen, F, U0, dep1, flags1)
    # mask only under the model
    gen.set_camera(F.CameraModel(*model))
    gen.set_depth_gate(None)
    gen.create_pointcloud(bgr, U0, 1, F.FEATURES_RGB)
    dep2, flags2 = G.gate(U, None, model[0], mask, qu, qv)
    _planes_equal(gen, F, U, dep2, flags2)
    gen.close()


def test_the_gate_reads_the_registered_plane(pkg):
    """rig K: k_fe_depth_final writes the plane the gate reads; then the same beside the distorting colour model A,
    whose map the mask follows while the depth does not"""
    F = pkg.frontend
    w, h, cam, rig = D.RIGS["K"]
    gate = G.make_gate(0.65, 1.9, 0.05, 1, 1)            # (the rig's scene: a box at 0.6 m before a wall from 1.2 m)
    bgr = G.frame(w, h, 72)
    raw = D.scene(pkg.data, rig)
    mask = G.mask_scene(w, h, 72)
    U = D.register(rig, cam, w, h, raw)
    dep, flags = G.gate(U, gate, cam[0], mask)
    for k in (G.MASKED, G.RANGE, G.JUMP):
        assert np.count_nonzero(flags == k) >= 1
    assert np.count_nonzero(dep) >= np.count_nonzero(U) // 4
    gen = _generator(pkg, w, h)
    gen.set_camera(F.CameraModel(*(cam + (ZERO,))))
    gen.set_depth_camera(D.to_struct(F, rig))
    gen.set_depth_gate(G.to_struct(F, gate))
    gen.set_mask(mask)
    gen.create_pointcloud(bgr, raw, 1, F.FEATURES_RGB)
    _planes_equal(gen, F, U, dep, flags)
    assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), raw)
    model = R.SMALL["A"][2]
    qu, qv = R.rectify_map(model, w, h)
    UA = D.register(rig, model[:5], w, h, raw)
    depA, flagsA = G.gate(UA, gate, model[0], mask, qu, qv)
    gen.set_camera(F.CameraModel(*model))
    gen.create_pointcloud(bgr, raw, 1, F.FEATURES_RGB)
    _planes_equal(gen, F, UA, depA, flagsA)
    gen.close()


# ---- 3. the cloud by bits ----------------------------------------------------------------------

CLOUD_GATE = dict(G.FULL, grow=1, hole_border=1)


def _cloud_frame(pkg, kind):
    if kind == "small":
        return G.frame(96, 64, 72), G.gate_scene(96, 64, 72, "blocks")
    if kind == "low":
        return low_texture_frame(pkg)[0], G.gate_scene(640, 480, 6, "blocks")
    return G.frame(640, 480, 72), G.gate_scene(640, 480, 72, "blocks")


@pytest.mark.parametrize("kind", ["small", "textured", "low"])
def test_cloud_by_bits(pkg, kind):
    """the oracle on (RECT_BGR, reference-gated depth) gives the device's cloud and map; selection is untouched:
    num_selected does not move, num_points drops.  "low": the Canny re-emit of collect() reads the gated plane too"""
    F = pkg.frontend
    bgr, U = _cloud_frame(pkg, kind)
    h, w = U.shape
    mask = G.mask_scene(w, h, 72)
    dep, flags = _ref(("cloud", kind), lambda: G.gate(U, CLOUD_GATE, G.SCALE, mask))
    gen = F.PcdGenerator(w, h) if kind != "small" else _generator(pkg, w, h)
    for ftype in (F.FEATURES_RGB, F.FEATURES_HSV):
        gen.set_depth_gate(None)
        gen.set_mask(None)
        gen.create_pointcloud(bgr, U, 1, ftype)
        plain = gen.info()
        gen.set_depth_gate(G.to_struct(F, CLOUD_GATE))
        gen.set_mask(mask)
        xyz, feat = gen.create_pointcloud(bgr, U, 1, ftype)
        _planes_equal(gen, F, U, dep, flags)
        ref = fo.create_pointcloud(gen.read_stage(F.STAGE_RECT_BGR), dep, 1, ftype, num_want=gen.num_want)
        info = gen.info()
        assert info["num_selected"] == ref["num_selected"] == plain["num_selected"]
        assert info["num_points"] == len(ref["positions"]) == len(xyz)
        assert 20 < info["num_points"] < plain["num_points"]
        assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
        assert _same_cloud((xyz, feat), (ref["positions"], ref["features"]))
        assert info["canny_used"] == plain["canny_used"] == (1 if kind == "low" else 0)
    gen.close()


# ---- 4. graphs and order -----------------------------------------------------------------------

def test_changes_of_gate_and_mask_on_one_context(pkg):
    """gate A, gate B, none, a mask, new contents of the mask, the mask cleared, on ONE context, a frame after each,
    through both feature types and both ways of taking the cloud: every plane is the reference's and every cloud the
    one a fresh context gives"""
    F = pkg.frontend
    w, h = 96, 64
    U = G.gate_scene(w, h, 73, "blocks")
    bgr = G.frame(w, h, 73)
    gate_a, gate_b = dict(G.FULL, grow=1), G.make_gate(0.0, 3.0, 0.08, 2, 1)
    mask1 = G.mask_scene(w, h, 73)
    mask2 = np.ascontiguousarray(mask1[::-1, ::-1])
    states = [(gate_a, None), (gate_b, None), (None, None), (None, mask1), (None, mask2), (None, None),
              (gate_b, mask2), (gate_a, mask2), (gate_a, None)]
    refs = [G.gate(U, g, G.SCALE, m) for g, m in states]
    for a, b in ((0, 1), (0, 2), (3, 4), (2, 3), (6, 7), (7, 8)):
        assert not np.array_equal(refs[a][1], refs[b][1])
    want = {}
    for ftype in (F.FEATURES_HSV, F.FEATURES_RGB):
        for k, (g, m) in enumerate(states):
            fresh = _generator(pkg, w, h)
            fresh.set_depth_gate(G.to_struct(F, g))
            fresh.set_mask(m)
            want[(ftype, k)] = fresh.create_pointcloud(bgr, U, 1, ftype)
            fresh.close()
            assert len(want[(ftype, k)][0]) > 20
    gen = _generator(pkg, w, h)
    for device_output in (False, True):
        gen.set_device_output(device_output)
        for rounds in range(2):
            for k, (g, m) in enumerate(states):
                ftype = F.FEATURES_HSV if (k + rounds) % 2 else F.FEATURES_RGB
                if rounds:                               # (either order of the two changes)
                    gen.set_mask(m); gen.set_depth_gate(G.to_struct(F, g))
                else:
                    gen.set_depth_gate(G.to_struct(F, g)); gen.set_mask(m)
                assert gen.depth_gate() == G.to_struct(F, g)
                assert _same_cloud(gen.create_pointcloud(bgr, U, 1, ftype), want[(ftype, k)])
                if g is None and m is None:
                    assert np.array_equal(gen.read_stage(F.STAGE_RECT_DEPTH), U)
                    assert np.array_equal(gen.read_stage(F.STAGE_UNGATED_DEPTH), U)
                    assert not gen.read_stage(F.STAGE_GATE).any()
                else:
                    _planes_equal(gen, F, U, *refs[k])
                gen.submit(bgr, U, 1, ftype)
                assert _same_cloud(gen.collect(), want[(ftype, k)])
                gen.submit(bgr, U, 1, ftype)
                _, _, n = gen.collect_device()
                assert n == len(want[(ftype, k)][0])
    gen.close()


def test_twenty_repeats_give_the_same_bytes(pkg):
    F = pkg.frontend
    w, h = 127, 193
    gate, U, mask, dep, flags = _case("mask+gate", w, h, 72)
    gen = _generator(pkg, w, h)
    gen.set_depth_gate(G.to_struct(F, gate))
    gen.set_mask(mask)
    bgr = G.frame(w, h, 72)
    first = None
    for _ in range(20):
        cloud = gen.create_pointcloud(bgr, U, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, U, dep, flags)
        first = first or cloud
        assert _same_cloud(cloud, first)
    gen.close()


# ---- 5. nothing changes without gate and mask --------------------------------------------------

def test_without_gate_and_mask_nothing_changes(pkg):
    F = pkg.frontend
    bgr, dep = pkg.data.synthetic_rgbd_frame(seed=72, texture=1.0)
    never = F.PcdGenerator(640, 480)
    want = {ft: never.create_pointcloud(bgr, dep, 1, ft) for ft in (F.FEATURES_RGB, F.FEATURES_HSV)}
    assert never.depth_gate() is None
    assert np.array_equal(never.read_stage(F.STAGE_UNGATED_DEPTH), never.read_stage(F.STAGE_RECT_DEPTH))
    assert np.array_equal(never.read_stage(F.STAGE_UNGATED_DEPTH), dep)
    assert not never.read_stage(F.STAGE_GATE).any()
    never.set_depth_gate(None)                          # clearing what was never set is no error
    never.set_mask(None)
    had = F.PcdGenerator(640, 480)
    had.set_depth_gate(F.DepthGate(0.8, 4.0, 0.05, 2, 1))
    had.set_mask(G.mask_scene(640, 480, 72))
    assert not _same_cloud(had.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want[F.FEATURES_RGB])
    had.set_depth_gate(None)
    had.set_mask(None)
    for ft, cloud in want.items():
        assert _same_cloud(had.create_pointcloud(bgr, dep, 1, ft), cloud) and len(cloud[0]) > 1000
        assert np.array_equal(had.read_stage(F.STAGE_RECT_DEPTH), dep)
        assert np.array_equal(had.read_stage(F.STAGE_UNGATED_DEPTH), dep)
        assert not had.read_stage(F.STAGE_GATE).any()
    # a gate whose tests are all off gates nothing
    had.set_depth_gate(F.DepthGate(grow=3))
    assert _same_cloud(had.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want[F.FEATURES_RGB])
    assert np.array_equal(had.read_stage(F.STAGE_RECT_DEPTH), dep) and not had.read_stage(F.STAGE_GATE).any()
    never.close(); had.close()


# ---- 6. refusals -------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable(pkg):
    F = pkg.frontend
    L = F.lib()
    w, h = 96, 64
    gate, U, mask, dep, flags = _case("mask+gate", w, h, 72)
    good = G.to_struct(F, gate)
    bgr = G.frame(w, h, 72)
    gen = _generator(pkg, w, h)
    gen.set_depth_gate(good)
    gen.set_mask(mask)
    want = gen.create_pointcloud(bgr, U, 1, F.FEATURES_RGB)
    assert len(want[0]) > 20
    u8p = C.POINTER(C.c_uint8)
    for g in G.bad_gates():
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_depth_gate(F.DepthGate(**g))
        assert gen.depth_gate() == good
    other = np.ascontiguousarray(mask[::-1])
    assert L.cvo_fe_set_mask(gen._h, other.ctypes.data_as(u8p), w - 1) != 0       # a stride below the width
    assert L.cvo_fe_set_mask(gen._h, other.ctypes.data_as(u8p), 0) != 0
    with pytest.raises(ValueError):
        gen.set_mask(mask[:, :-1])
    assert _same_cloud(gen.create_pointcloud(bgr, U, 1, F.FEATURES_RGB), want)
    _planes_equal(gen, F, U, dep, flags)
    # while a frame is submitted and not collected both setters refuse, set and clear; the frame arrives intact
    gen.submit(bgr, U, 1, F.FEATURES_RGB)
    for call in (lambda: gen.set_depth_gate(F.DepthGate(0.5, 3.0)), lambda: gen.set_depth_gate(None),
                 lambda: gen.set_mask(other), lambda: gen.set_mask(None)):
        with pytest.raises(pkg.capi.CvoHipError):
            call()
    assert _same_cloud(gen.collect(), want)
    _planes_equal(gen, F, U, dep, flags)
    assert gen.depth_gate() == good
    # ... and afterwards they are accepted; a mask with padded rows and a bool mask are the same mask
    padded = np.zeros((h, w + 5), np.uint8)
    padded[:, :w] = other
    gen.set_mask(padded[:, :w])
    gen.create_pointcloud(bgr, U, 1, F.FEATURES_RGB)
    _planes_equal(gen, F, U, *G.gate(U, gate, G.SCALE, other))
    gen.set_mask(other != 0)
    gen.create_pointcloud(bgr, U, 1, F.FEATURES_RGB)
    _planes_equal(gen, F, U, *G.gate(U, gate, G.SCALE, other))
    # a context that never had a gate stays without one
    fresh = _generator(pkg, w, h)
    table = fresh.create_pointcloud(bgr, U, 1, F.FEATURES_RGB)
    for g in G.bad_gates():
        with pytest.raises(pkg.capi.CvoHipError):
            fresh.set_depth_gate(F.DepthGate(**g))
    assert L.cvo_fe_set_mask(fresh._h, other.ctypes.data_as(u8p), w - 1) != 0
    assert fresh.depth_gate() is None
    assert _same_cloud(fresh.create_pointcloud(bgr, U, 1, F.FEATURES_RGB), table)
    assert not fresh.read_stage(F.STAGE_GATE).any()
    fresh.close(); gen.close()


def test_a_refused_gate_takes_no_memory(pkg):
    """On a context of 2048 x 2048 the ungated plane and the flags are 12 MiB and the mask 4 MiB more.  A context
    that never set a gate, refused gates and a refused mask leave the free device memory where it was, to the 8 MiB
    such a reading resolves; an accepted gate is seen by the same reading."""
    import torch
    F = pkg.frontend
    L = F.lib()
    n = 2048
    gen = F.PcdGenerator(n, n)
    mask = np.zeros((n, n), np.uint8)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for g in G.bad_gates():
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_depth_gate(F.DepthGate(**g))
    assert L.cvo_fe_set_mask(gen._h, mask.ctypes.data_as(C.POINTER(C.c_uint8)), n - 1) != 0
    gen.set_depth_gate(None)
    gen.set_mask(None)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 * 1024 * 1024, "refused calls took %d bytes" % (free0 - free1)
    assert gen.depth_gate() is None
    gen.set_depth_gate(F.DepthGate(0.8, 4.0, 0.05, 1))
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert free1 - free2 >= 8 * 1024 * 1024, "an accepted gate took only %d bytes" % (free1 - free2)
    gen.close()


def test_a_closed_context_gives_every_optional_buffer_back(pkg):
    """Four rounds of: a context of 2048 x 2048, a distorting camera, a depth camera of 2048 x 2048, a gate, a mask,
    close.  The smallest buffer any of them brings (the flags, the mask) is 4 MiB, so one that close() forgot would
    cost 16 MiB over the rounds: the free device memory is where it was, to the 8 MiB such a reading resolves.
    One such round runs in front of the first reading: what the runtime takes once per process with the first
    context (a process that starts with this test: about 150 MiB) is not the context's."""
    import torch
    F = pkg.frontend
    n = 2048
    cam = (5000.0, 1700.0, 1700.0, 1024.0, 1024.0)
    mask = np.zeros((n, n), np.uint8)

    def one_round():
        gen = F.PcdGenerator(n, n)
        gen.set_camera(F.CameraModel(*(cam + ((0.05, -0.02, 0.001, 0.001, 0.0),))))
        gen.set_depth_camera(D.to_struct(F, D.identity_rig(n, n, cam)))
        gen.set_depth_gate(F.DepthGate(0.8, 4.0, 0.05, 1))
        gen.set_mask(mask)
        gen.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    free = [one_round() for _ in range(5)]
    print("free device memory after each round:", free)
    assert abs(free[0] - free[4]) < 8 * 1024 * 1024, "four closed contexts left %d bytes taken" % (free[0] - free[4])


# ---- 7. the layers above -----------------------------------------------------------------------

RUN_GATE = dict(G.FULL, grow=1, hole_border=1)


def _frames(pkg):
    return _four_frames(pkg, 75, lambda k, dep: G.gate_scene(640, 480, 75 + k, "blocks"))


def test_run_frames_with_a_gate_and_a_mask(pkg):
    """run_frames(depth_gate=, mask=) on the raw frames = the generator driven by hand = run_frames without either
    on the reference-gated frames: the same poses"""
    F = pkg.frontend
    frames = _frames(pkg)
    mask = G.mask_scene(640, 480, 75)
    gated = [(name, bgr, _ref(("seq", k), lambda: G.gate(dep, RUN_GATE, G.SCALE, mask))[0])
             for k, (name, bgr, dep) in enumerate(frames)]
    poses = []
    for fr, gate, m in ((frames, G.to_struct(F, RUN_GATE), mask), (gated, None, None)):
        reg = pkg.Cvo()
        buf = io.StringIO()
        assert F.run_frames(reg, fr, 1, writer=pkg.trajectory.TrajectoryWriter(buf), depth_gate=gate, mask=m) == 4
        poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
        reg.close()
    # by hand
    reg = pkg.Cvo()
    buf = io.StringIO()
    writer = pkg.trajectory.TrajectoryWriter(buf)
    gen = F.PcdGenerator(640, 480)
    gen.set_depth_gate(G.to_struct(F, RUN_GATE))
    gen.set_mask(mask)
    gen.set_device_output(True)
    for k, (name, bgr, dep) in enumerate(frames):
        gen.submit(bgr, dep, 1, F.FEATURES_RGB)
        dp, df, n = gen.collect_device()
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == gated[k][2].tobytes()
        reg.run_cvo_device(dp, df, n)
        writer.append(name, reg.accum_transform)
    poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
    reg.close(); gen.close()
    for p in poses[1:]:
        assert p[0] == poses[0][0] and np.array_equal(p[1], poses[0][1]) and p[2] == poses[0][2] > 0
    assert len(poses[0][0].strip().split("\n")) == 4


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_a_gate_and_a_mask(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_depth_gate / clear_depth_gate / set_mask / clear_mask
    (tests/cpp/cvo_depth_gate_demo.cpp): the clouds the C++ object registers and its pose lines equal the Python path's"""
    F = pkg.frontend
    w, h = 640, 480
    frames = _frames(pkg)
    gate = G.to_struct(F, RUN_GATE)
    mask = G.mask_scene(w, h, 75)
    got = _demo_lines(tmp_path, "cvo_depth_gate_demo", frames, w, h, bytes(gate) + mask.tobytes(), [mode_name])
    gen = F.PcdGenerator(w, h)

    def prepare(k):
        gen.set_depth_gate(None if k == 2 else gate)
        gen.set_mask(None if k == 2 else mask)
        return ["refused a bad gate"] if k == 3 else []

    want, sizes, _ = _device_path_lines(pkg, mode_name, gen, frames, prepare)
    assert got == ["refused a bad gate", "refused a mask without a size"] + want
    ftype = F.FEATURES_HSV if mode_name == "acvo" else F.FEATURES_RGB
    # the gated frames' clouds are the oracle's on the reference-gated depth, and smaller than the ungated frame's
    rd = G.gate(frames[0][2], RUN_GATE, G.SCALE, mask)[0]
    assert sizes[0] == len(fo.create_pointcloud(frames[0][1], rd, 1, ftype)["positions"]) > 100
    assert sizes[2] > max(sizes[0], sizes[1], sizes[3])
    gen.close()
