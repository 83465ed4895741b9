"""What the GPU tests of the front end share (test_gpu_frontend.py, test_gpu_fe_rectify.py, test_gpu_fe_depth.py,
test_gpu_fe_gate.py): clouds compared by bits, the four frames of the layer tests, and the C++ demos of tests/cpp --
their input file, their build and run, and the restatements of what they print."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_cloud(got, want):
    return (got[0].shape == want[0].shape and np.array_equal(_bits(got[0]), _bits(want[0])) and
            np.array_equal(_bits(got[1]), _bits(want[1])))


def _four_frames(pkg, seed, depth=None):
    """Four frames (name, bgr, depth) of one scene in motion, named like a TUM sequence.  `depth(k, dep)` gives
    frame k's depth image in place of the synthetic one."""
    out = []
    for k in range(4):
        bgr, dep = pkg.data.synthetic_rgbd_frame(seed=seed, texture=1.0, motion=(1.2 * k, -0.6 * k))
        out.append(("1305031453.%06d" % (359684 + 33333 * k), bgr, dep if depth is None else depth(k, dep)))
    return out


def _digest(a):
    """fe_demo_common.hpp's digest of an array of rows: modulo 2^64, whatever the order of the rows"""
    w = np.ascontiguousarray(a).view(np.uint32).astype(np.uint64)
    h = (w * np.arange(1, w.shape[1] + 1, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return int((h * h).sum(dtype=np.uint64))


def _pose_line_f32(name, M):
    """The pose line as the C++ object prints it: the translation and Affine3f::quaternion of cvo_class.cpp (Eigen's
    quaternion-from-matrix, every operation in float32, in that order) of the float32 matrix, each as a default
    std::ostream prints a float (%g).  data.pose_line forms the quaternion in float64 from the same matrix, so its sixth
    digit may differ; this restatement is what the demo's text is compared with, character for character."""
    f = np.float32
    m = np.asarray(M)
    assert m.dtype == np.float32 and m.shape == (4, 4)
    m = m.reshape(16)
    t = (m[0] + m[5]) + m[10]
    if t > f(0.0):
        t = np.sqrt(t + f(1.0))
        w = f(0.5) * t
        t = f(0.5) / t
        x, y, z = (m[9] - m[6]) * t, (m[2] - m[8]) * t, (m[4] - m[1]) * t
    else:
        i = 0
        if m[5] > m[0]:
            i = 1
        if m[10] > m[5 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(((m[5 * i] - m[5 * j]) - m[5 * k]) + f(1.0))
        q = [f(0.0)] * 3
        q[i] = f(0.5) * t
        t = f(0.5) / t
        w = (m[4 * k + j] - m[4 * j + k]) * t
        q[j] = (m[4 * j + i] + m[4 * i + j]) * t
        q[k] = (m[4 * k + i] + m[4 * i + k]) * t
        x, y, z = q
    vals = [m[3], m[7], m[11], x, y, z, w]
    assert all(type(v) is np.float32 for v in vals)
    return "%s %s" % (name, " ".join("%g" % float(v) for v in vals))


def _demo_lines(tmp_path, demo, frames, w, h, settings=b"", args=(), depth_sizes=False):
    """Builds tests/cpp/<demo>.cpp against the library, writes its frames.bin and returns the lines it prints.
    The file: int32 n_frames, width, height; `settings` (what the demo reads in front of the frames); per frame 32
    bytes of name, the colour image and the depth image, the latter behind its int32 width and height when
    `depth_sizes`."""
    exe = str(tmp_path / demo)
    lib = os.path.join(ROOT, "cvo-rgbd_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", demo + ".cpp"), "-L", lib, "-lcvo_hip",
                    "-Wl,-rpath," + lib, "-o", exe], check=True, timeout=120)
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<iii", len(frames), w, h))
        fh.write(settings)
        for name, bgr, dep in frames:
            fh.write(name.encode().ljust(32, b"\0"))
            fh.write(bgr.tobytes())
            if depth_sizes:
                fh.write(struct.pack("<ii", dep.shape[1], dep.shape[0]))
            fh.write(dep.tobytes())
    out = subprocess.run([exe, path] + list(args), check=True, capture_output=True, text=True, timeout=120).stdout
    return out.strip().split("\n")


def _device_path_lines(pkg, mode_name, gen, frames, prepare):
    """What a demo prints for `frames`, from the Python path with the hand-over the C++ object uses (device memory):
    per frame `prepare(k)` sets the generator up and returns the lines the demo prints in front of that frame, then
    the cloud line and the pose line.  Returns (lines, points per frame, [(name, accumulated transform)])."""
    F = pkg.frontend
    acvo = mode_name == "acvo"
    reg = (pkg.Acvo if acvo else pkg.Cvo)()
    gen.set_device_output(True)
    ftype = F.FEATURES_HSV if acvo else F.FEATURES_RGB
    lines, sizes, poses = [], [], []
    for k, (name, bgr, dep) in enumerate(frames):
        lines += prepare(k)
        gen.submit(bgr, dep, 1, ftype)
        dp, df, n = gen.collect_device()
        sizes.append(n)
        reg.run_cvo_device(dp, df, n)
        d = reg.ctx.device_cloud(0)
        assert d["points"] == n
        lines.append("cloud %s %d %d %d" % (name, n, _digest(d["pos"][:n]), _digest(d["feat"][:n])))
        lines.append(_pose_line_f32(name, reg.accum_transform))
        poses.append((name, reg.accum_transform.copy()))
    lines.append("points_last_frame %d iterations %d" % (sizes[-1], reg.num_iterations))
    reg.close()
    return lines, sizes, poses
