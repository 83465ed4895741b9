"""CPU: the pair <-> (entry, bit) map of the tile lists (csrc/cvo_device.h tile_pair / tile_key) is host-and-device code:
expand_lists expands an entry's mask with it, k_tiles_from_record rebuilds a list from its candidate record with the inverse.
tests/cpp/tile_key_host.cpp holds the two to each other for every result register and bit, at the first tiles and at the last
tiles of clouds of 10 000 and 65 536 rows, and rebuilds entries from subsets of their 64 pairs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_key_inverts_the_expansion(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the map's header needs the HIP headers")
    exe = str(tmp_path / "tile_key_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-invalid-offsetof",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cvo-rgbd_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "tile_key_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("ok")
