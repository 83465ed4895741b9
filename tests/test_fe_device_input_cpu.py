"""CPU: what device input does before a device is touched.  frontend.device_image against dummy objects with
`__cuda_array_interface__` (nothing is read through their pointers), the symbols against the header, and the extent
arithmetic of csrc/cvo_input.h in a program of its own under the host sanitizers.  No GPU:
tests/test_gpu_fe_device_input.py holds device frames to host frames by bits."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x7F0000001000


class Dummy:
    """an object with the interface and nothing behind it"""

    def __init__(self, shape, typestr, strides=None, ptr=PTR):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2,
                                         "strides": strides}


def test_the_symbols_and_the_header(pkg):
    F = pkg.frontend
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    for name in ("cvo_fe_submit_device", "cvo_fe_submit_stereo_device"):
        assert name in F.SYMBOLS and re.search(r"\bint %s\(" % name, text), name
    assert "THE DEVICE-INPUT CONTRACT" in text and "hipMemoryTypeDevice" in text and "LiDAR frames are out of scope" in text
    assert "device_input" in inspect.signature(F.run_frames).parameters
    assert callable(F.PcdGenerator.submit_device) and callable(F.PcdGenerator.submit_stereo_device)
    assert list(inspect.signature(F.device_image).parameters) == ["obj", "rows", "row_bytes", "itemsize", "what"]
    for doc in (F.PcdGenerator.submit_device.__doc__, F.run_frames.__doc__):
        assert "stream" in doc and "synchronis" in doc


def test_dense_images(pkg):
    dev = pkg.frontend.device_image
    assert dev(Dummy((48, 64, 3), "|u1"), 48, 192, 1, "img") == (PTR, 192)
    assert dev(Dummy((48, 64, 3), "|u1", strides=(192, 3, 1)), 48, 192, 1, "img") == (PTR, 192)
    assert dev(Dummy((48, 192), "<u1", strides=None), 48, 192, 1, "img") == (PTR, 192)           # packed rows
    assert dev(Dummy((72, 64), "|u1"), 72, 64, 1, "nv12") == (PTR, 64)
    assert dev(Dummy((48, 64), "<u2"), 48, 128, 2, "depth") == (PTR, 128)
    assert dev(Dummy((48, 64), "<f2", strides=(128, 2)), 48, 128, 2, "depth") == (PTR, 128)
    assert dev(Dummy((48, 64), "<f4", strides=(256, 4)), 48, 256, 4, "depth") == (PTR, 256)
    # one row: its stride does not count
    assert dev(Dummy((1, 64), "<f4", strides=(4, 4)), 1, 256, 4, "depth") == (PTR, 256)


def test_pitched_images(pkg):
    dev = pkg.frontend.device_image
    assert dev(Dummy((48, 64, 3), "|u1", strides=(200, 3, 1)), 48, 192, 1, "img") == (PTR, 200)
    assert dev(Dummy((48, 64, 3), "|u1", strides=(193, 3, 1)), 48, 192, 1, "img") == (PTR, 193)  # (bytes: any pitch)
    assert dev(Dummy((72, 64), "|u1", strides=(128, 1)), 72, 64, 1, "nv12") == (PTR, 128)
    assert dev(Dummy((48, 64), "<u2", strides=(130, 2)), 48, 128, 2, "depth") == (PTR, 130)
    assert dev(Dummy((48, 64), "<f4", strides=(260, 4), ptr=PTR + 4), 48, 256, 4, "depth") == (PTR + 4, 260)


@pytest.mark.parametrize("obj, args", [
    (Dummy((48, 64, 3), "<f4"), (48, 192, 1)),                           # a wrong dtype
    (Dummy((48, 64, 3), "|i1"), (48, 192, 1)),
    (Dummy((48, 64), "<u4"), (48, 256, 4)),
    (Dummy((48, 64), "<f8"), (48, 256, 4)),
    (Dummy((48, 64), ">u2"), (48, 128, 2)),                              # the other byte order
    (Dummy((48, 64), "<f4"), (48, 128, 2)),
    (Dummy((48, 63, 3), "|u1"), (48, 192, 1)),                           # a wrong shape
    (Dummy((47, 64, 3), "|u1"), (48, 192, 1)),
    (Dummy((48 * 64 * 3,), "|u1"), (48, 192, 1)),                        # (one dimension: no rows)
    (Dummy((64, 48), "<u2"), (48, 128, 2)),
    (Dummy((48, 64, 3), "|u1", strides=(192, 6, 2)), (48, 192, 1)),      # a last dimension that is not dense
    (Dummy((48, 64), "<u2", strides=(256, 4)), (48, 128, 2)),
    (Dummy((48, 64, 3), "|u1", strides=(400, 6, 1)), (48, 192, 1)),      # ... or a middle one
    (Dummy((48, 64, 3), "|u1", strides=(191, 3, 1)), (48, 192, 1)),      # a pitch below the row
    (Dummy((48, 64), "<f4", strides=(252, 4)), (48, 256, 4)),
    (Dummy((48, 64), "<u2", strides=(0, 2)), (48, 128, 2)),
    (Dummy((48, 64), "<u2", strides=(131, 2)), (48, 128, 2)),            # an odd pitch for 2-byte items
    (Dummy((48, 64), "<f2", strides=(129, 2)), (48, 128, 2)),
    (Dummy((48, 64), "<f4", strides=(258, 4)), (48, 256, 4)),            # ... and one that is no multiple of 4
    (Dummy((48, 64), "<f4", strides=(257, 4)), (48, 256, 4)),
    (Dummy((48, 64, 3), "|u1", strides=(-192, 3, 1)), (48, 192, 1)),     # negative strides
    (Dummy((48, 64), "<u2", strides=(128, -2)), (48, 128, 2)),
    (Dummy((48, 64), "<u2", strides=(128,)), (48, 128, 2)),              # strides of another rank
    (Dummy((48, 64), "<u2", ptr=0), (48, 128, 2)),                       # a null pointer
    (object(), (48, 128, 2)),                                            # no interface at all
])
def test_what_device_image_refuses(pkg, obj, args):
    with pytest.raises(ValueError, match="^the image: "):
        pkg.frontend.device_image(obj, *args, "the image")


def test_the_snippet_of_the_integration_guide_compiles(tmp_path):
    """the C++ of INTEGRATION section 8's device-input part in front of a compiler, against the two headers and the HIP
    runtime's: a typo check of names, argument counts and pointer types; it pins nothing about results"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    part = text[text.index("### Frames already on the device"):text.index("## 9. ")]
    blocks = re.findall(r"```cpp\n(.*?)```", part, re.S)
    assert len(blocks) == 1 and "cvo_fe_submit_device(" in blocks[0] and "cvo_fe_set_depth_format(" in blocks[0]
    assert "THE STREAM RULE" in part and "THE DEPTH-FORMAT CONTRACT" in part and "THE DEVICE-INPUT CONTRACT" in part
    src = tmp_path / "snippet.cpp"
    src.write_text(blocks[0])
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    built = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I",
                            os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"), str(src)],
                           capture_output=True, text=True, timeout=120)
    assert built.returncode == 0, built.stderr[-3000:]


def test_the_extent_arithmetic_under_the_host_sanitizers(tmp_path):
    """tests/cpp/input_extent_host.cpp drives csrc/cvo_input.h in a process of its own, built with the host compiler and
    -fsanitize=address,undefined; plain where the sanitizer runtime does not link"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "tests", "cpp", "input_extent_host.cpp")
    exe = str(tmp_path / "input_extent_host")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "cvo-rgbd_amd", "csrc"), src, "-o", exe]
    # (the runtimes linked into the program itself: it then starts under whatever the environment preloads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) != "clang++" else []
    built = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static, capture_output=True,
                           text=True)
    if built.returncode != 0:
        print("the sanitizer runtime does not link here; built plain:", built.stderr[-300:])
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout.strip())
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
