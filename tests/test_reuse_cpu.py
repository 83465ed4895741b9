"""CPU: the re-use bounds of the list plans far from the origin, without a GPU.

(a) tests/cpp/reuse_host.cpp drives the library's own host-and-device plan (csrc/cvo_device.h prepare_iteration: plan_lists,
    plan_xy_async, plan_self_async_one; pose_travel, xy_travel, apply_tf) over an extremal stream of single pairs: a build, then
    a change of pose -- or, for the yy list of acvo, a growth of the length scale -- that uses up all but 0 - 0.2 % of what the
    plan still allows and brings the pair to sqrt(tau) +- four ulp of the coordinates.  No trial may have the plan name re-use
    or a narrowing while a member of A is absent from the tile list or the record; pose_travel and xy_travel must bound the
    float64 displacement; and the driver's own floors keep it from passing empty (>= 90 % of the trials of a class re-use;
    from 1.5 km on >= 200 trials of a class hold a member under a re-used list).  40 classes (8 offsets x 5 plans) of 6 000
    trials, two seconds.

    What it found.  With the slack the plans had before reuse_slack, 1e-4 (1 + xmax + y0max) whatever the coordinates, the
    same stream loses members from 1.5 km on in every plan (DESIGN.md section 3 has the table: 79 of 119 654 trials with a
    member under a re-used list, none nearer than 1.5 km); with reuse_slack it loses none.

(b) The oracle's grid search against its dense search on the registrations tests/test_gpu_reuse_far.py holds the device to:
    far150 .. far3700 with the break tests off, 40 iterations each (hostile_cases.long_params).  The grid is the arbiter
    there and had been checked far from the origin for 1 - 7 iterations only."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_cases as hc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIALS = 6000   # per class (offset x plan)
PLANS = ("sync", "narrow", "async", "yy", "yy-async")
OFFSETS = ("(0, 0, 1.5)", "(80, -120, 60)", "(300, -500, 200)", "(800, -1200, 600)", "(2000, -3000, 1500)", "(1024, -2048, 512)",
           "(2048, -4096, 1024)", "(3000, 0, 0)")
FAR_OFFSETS = OFFSETS[3:]


@pytest.fixture(scope="module")
def reuse_host(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the plan's header needs the HIP headers")
    exe = str(tmp_path_factory.mktemp("reuse") / "reuse_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-invalid-offsetof",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cvo-rgbd_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "reuse_host.cpp"), "-o", exe], check=True)
    return exe


def _per_class(stdout):
    """{(offset text, plan): [trials, re-use, members under re-use, lost]} summed over the length scales."""
    out = {}
    for line in stdout.splitlines():
        if not line.startswith("offset"):
            continue
        key = (line[line.index("("):line.index(")") + 1], line.split(" plan ")[1].split()[0])
        tok = line.replace(",", "").split()
        got = [int(tok[tok.index("trials") - 1]), int(tok[tok.index("re-use") - 1]), int(tok[tok.index("with") - 1]), int(tok[tok.index("lost") - 1])]
        out[key] = [a + b for a, b in zip(out.get(key, [0, 0, 0, 0]), got)]
    return out


def test_no_plan_reuses_a_list_that_lacks_a_member(reuse_host):
    r = subprocess.run([reuse_host, str(TRIALS)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    per = _per_class(r.stdout)
    assert sorted(per) == sorted((o, p) for o in OFFSETS for p in PLANS)
    members = 0
    for key, (trials, reuse, member, lost) in per.items():
        assert trials == TRIALS, key
        assert 10 * reuse >= 9 * trials, (key, reuse, trials)          # the plan names re-use in at least 90 % of a class
        if key[0] in FAR_OFFSETS:
            assert member >= 200, (key, member)                         # ... and far out the re-used lists are asked for members
        assert lost == 0, (key, lost, member)
        members += member
    assert "travel bounds: 0 failed of" in r.stdout and "floors missed: 0" in r.stdout
    assert r.returncode == 0 and r.stdout.strip().endswith("lost 0 of %d" % members)


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
@pytest.mark.parametrize("name", hc.REUSE_NAMES)
def test_oracle_grid_search_equals_dense_over_40_iterations(pkg, po, name, mode_name):
    acvo = mode_name == "acvo"
    n_g, tr_g, st_g = hc.oracle_long_align(po, pkg.data, name, acvo, po.SEARCH_GRID)
    n_d, tr_d, st_d = hc.oracle_long_align(po, pkg.data, name, acvo, po.SEARCH_DENSE)
    print(name, mode_name, "iterations", n_g, "nnz", [t["nnz"] for t in tr_g], "ell", [round(float(t["ell"]), 4) for t in tr_g])
    assert n_g == n_d == hc.REUSE_ITERATIONS, (n_g, n_d)   # the break tests are off: the lists get re-used
    assert len(tr_g) == len(tr_d) == n_g
    for k, (a, b) in enumerate(zip(tr_g, tr_d)):
        assert a["nnz"] == b["nnz"] and a["ell"] == b["ell"], (name, mode_name, k, a["nnz"], b["nnz"])
        assert a["omega"] == b["omega"] and a["v"] == b["v"] and a["step"] == b["step"], (name, mode_name, k)
        assert a["nnz"] > 0, (name, mode_name, k)
    assert st_g == st_d
    if not acvo:   # cvo walks its whole schedule
        assert [float(tr_g[k]["ell"]) for k in (0, 5, 15, 39)] == [float(np.float32(x)) for x in (0.15, 0.10, 0.06, 0.03)]
