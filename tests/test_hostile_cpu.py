"""CPU: the hostile geometry of tests/hostile_cases.py, without a GPU.

(a) The oracle's grid search against its dense search on every case, pose and length scale: the grid is the arbiter of
    the -m gpu tests (tests/test_gpu_hostile.py) and had never been checked far from the origin.
(b) The bounding-sphere cull of k_filter with the library's own host-and-device code (csrc/cvo_device.h spheres_near,
    cull_slack, apply_tf, compute_filter_bounds), driven by tests/cpp/cull_host.cpp over the extremal stream of
    test_gpu_hostile.py: 21 000 trials per offset class, none may have a member of A in a culled pair of runs.

What (b) found.  With the bound as it was before cull_slack (reach = sqrt(tauf): a slack of 1e-5 relative + 1e-5 m that
does not grow with the coordinates), the same stream loses members from 600 m on:
    offset (0, 0, 1.5)          0 lost of 20 367 trials with a member
    offset (80, -120, 60)       0 of 14 174
    offset (300, -500, 200)    23 of 14 497   (0.16 %)
    offset (800, -1200, 600)   83 of 13 564   (0.61 %)
    offset (2000, -3000, 1500) 29 of 14 344   (0.20 %)
(profiles/r08_ab.txt).  The second test keeps that visible: the stream must stay sharp enough to catch the old bound.

The spheres (b) culls with are cull_host.cpp's own restatement of k_cloud_seg (run_sphere).  That the device's spheres are
those -- centre, radius and padding by bits, and every live row inside its run's sphere -- is pinned by
tests/test_gpu_cloud_layout.py against tests/cloud_layout_ref.py."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_cases as hc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIALS = 7000   # per (offset, largest angle): 21 000 per offset class


@pytest.fixture(scope="module")
def data(pkg):
    return pkg.data


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
@pytest.mark.parametrize("name", hc.NAMES)
def test_oracle_grid_search_equals_dense(po, data, name, mode_name):
    acvo = mode_name == "acvo"
    p = po.default_params(po.MODE_ACVO if acvo else po.MODE_CVO)
    xf, ff, xm, fm = hc.clouds(data, name, acvo)
    total = 0
    for label, R, T in hc.poses(xf):
        y = po.transform(R, T, xm)
        for ell in hc.ELLS:
            grid = po.se_kernel(p, ell, xf, ff, y, fm, search=po.SEARCH_GRID)
            dense = po.se_kernel(p, ell, xf, ff, y, fm, search=po.SEARCH_DENSE)
            for g, d in zip(grid, dense):
                assert np.array_equal(g, d), (name, label, ell)
            total += len(grid[1])
            if name in hc.FAR:   # a rotation about the origin would have emptied these
                assert len(grid[1]) > 0, (name, label, ell)
    if not name.startswith("tiny"):
        assert total > 0, name


@pytest.fixture(scope="module")
def cull_host(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the cull's header needs the HIP headers")
    exe = str(tmp_path_factory.mktemp("cull") / "cull_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-invalid-offsetof",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cvo-rgbd_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "cull_host.cpp"), "-o", exe], check=True)
    return exe


def _lost_per_offset(stdout):
    """{offset text: (lost, trials with a member)} summed over the angles."""
    out = {}
    for line in stdout.splitlines():
        if not line.startswith("offset"):
            continue
        key = line[line.index("("):line.index(")") + 1]
        tok = line.split()
        lost, members = int(tok[tok.index("lost") - 1]), int(tok[tok.index("with") - 1])
        a, b = out.get(key, (0, 0))
        out[key] = (a + lost, b + members)
    return out


def test_cull_keeps_every_member_on_the_extremal_stream(cull_host):
    r = subprocess.run([cull_host, str(TRIALS), "1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    per = _lost_per_offset(r.stdout)
    assert len(per) == len(hc.CULL_CLASSES)
    for key, (lost, members) in per.items():
        assert members >= 3 * TRIALS // 2, (key, members)   # at least half the trials of a class hold a member
        assert lost == 0, (key, lost, members)
    assert r.returncode == 0 and r.stdout.strip().endswith("lost 0 of %d" % sum(m for _, m in per.values()))


def test_the_stream_catches_a_slack_that_ignores_the_coordinates(cull_host):
    """The same trials against reach = sqrt(tauf), the cull before cull_slack: members are lost from 600 m on (the module
    docstring has the counts), none near the origin.  A stream that no longer shows this no longer tests the slack."""
    r = subprocess.run([cull_host, str(TRIALS), "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    per = _lost_per_offset(r.stdout)
    assert r.returncode == 1
    assert per["(0, 0, 1.5)"][0] == 0
    for key in ("(300, -500, 200)", "(800, -1200, 600)", "(2000, -3000, 1500)"):
        assert per[key][0] > 0, (key, per[key])
