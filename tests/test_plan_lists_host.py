"""CPU: plan_lists (csrc/cvo_device.h) is host-and-device code; tests/cpp/plan_lists_host.cpp steps it through cvo's
length-scale schedule on two small clouds with a synthetic motion and keeps a float64 model of the tile list and of the
candidate record.  Whenever the plan names re-use or a narrowing (option `record_narrow`), record and tile list must hold
every pair inside the kernel's radius at the current pose; with the option off the plan is the old one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_lists_keeps_every_member_when_it_reuses_or_narrows(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the plan's header needs the HIP headers")
    exe = str(tmp_path / "plan_lists_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-invalid-offsetof",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cvo-rgbd_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "plan_lists_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("ok")
