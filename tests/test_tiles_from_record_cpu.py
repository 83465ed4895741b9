"""CPU: the rule by which an engine's xy tile list is replaced by its candidate record's pair set (csrc/cvo_device.h
record_covers_its_radius, plan_lists with DevParams::list_stale_engine) is host-and-device code.  tests/cpp/tiles_from_record_host.cpp
steps the plan through cvo's length-scale schedule on two small clouds with a synthetic motion and launch geometries that change every
1 to 11 iterations, keeps a float64 model of tile list and record, rebuilds the list from the record where the rule allows it, and
asserts in every iteration that both hold every pair inside the kernel's radius at the current pose."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rebuilt_lists_keep_every_member(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the plan's header needs the HIP headers")
    exe = str(tmp_path / "tiles_from_record_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-invalid-offsetof",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cvo-rgbd_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "tiles_from_record_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("ok")
