"""CPU: the host-only half of the unpack contract (cvo_fe_check_pixel_format, cvo_fe_pixel_layout) against the layout
table of tests/fe_unpack_ref.py; the facts the contract states about its own arithmetic (the anchors, the grey axis, the
accumulator bound, flat colours and ramps through the demosaic); what the inputs of the GPU test are; and which errors
of a device implementation (tests/fe_unpack_mutants.py) they tell from the restatement.  No GPU:
tests/test_gpu_fe_unpack.py holds k_fe_unpack to the same restatement by bytes."""
import inspect
import os
import re

import numpy as np
import pytest

import fe_unpack_mutants as M
import fe_unpack_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = (1, 2, 3, 64, 65, 8192)


def test_the_constants_and_the_symbols(pkg):
    F = pkg.frontend
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    for k, name in enumerate(K.NAMES):
        assert getattr(F, "PIXEL_" + name) == k == getattr(K, name)
        assert re.search(r"\bCVO_FE_PIXEL_%s = %d\b" % (name, k), text), name
    assert (F.STAGE_INPUT_BGR, F.STAGE_INPUT_RIGHT_BGR) == (30, 31)
    assert re.search(r"\bCVO_FE_STAGE_INPUT_BGR = 30\b", text) and re.search(r"\bCVO_FE_STAGE_INPUT_RIGHT_BGR = 31\b", text)
    for name in ("cvo_fe_check_pixel_format", "cvo_fe_pixel_layout", "cvo_fe_set_pixel_format", "cvo_fe_get_pixel_format",
                 "cvo_fe_unpack_image"):
        assert name in F.SYMBOLS and re.search(r"\bint %s\(" % name, text), name
    assert "pixel_format" in inspect.signature(F.run_frames).parameters
    assert callable(F.PcdGenerator.set_pixel_format) and callable(F.PcdGenerator.pixel_format)


@pytest.mark.parametrize("fmt", K.FORMATS, ids=K.NAMES)
def test_check_and_layout_against_the_table(pkg, fmt):
    F = pkg.frontend
    bpp = {"BGR8": 3, "RGB8": 3, "BGRA8": 4, "RGBA8": 4, "YUY2": 2, "UYVY": 2}.get(K.NAMES[fmt], 1)
    for w in SIDES:
        for h in SIDES:
            want = K.layout(fmt, w, h)
            assert F.check_pixel_format(fmt, w, h) == (want is not None), (w, h)
            if want is None:
                with pytest.raises(pkg.capi.CvoHipError):
                    F.pixel_layout(fmt, w, h)
                continue
            assert F.pixel_layout(fmt, w, h) == want == ((h + h // 2) if fmt == K.NV12 else h, w * bpp), (w, h)
    # what the sizes say, spelled out
    even_w, even_h, two = fmt in K.YUV, fmt == K.NV12, fmt in K.BAYER
    assert F.check_pixel_format(fmt, 65, 64) == (not even_w) and F.check_pixel_format(fmt, 64, 65) == (not even_h)
    assert F.check_pixel_format(fmt, 1, 64) == (not even_w and not two) and F.check_pixel_format(fmt, 64, 1) == (not even_h and not two)
    assert not F.check_pixel_format(fmt, 0, 64) and not F.check_pixel_format(fmt, 64, 0) and not F.check_pixel_format(fmt, -2, -2)


def test_unknown_formats_and_null_pointers_are_refused(pkg):
    F = pkg.frontend
    L = F.lib()
    for bad in (-1, 12, 2 ** 31 - 1):
        assert not F.check_pixel_format(bad, 64, 64)
        with pytest.raises(pkg.capi.CvoHipError):
            F.pixel_layout(bad, 64, 64)
    import ctypes as C
    row, rows = C.c_size_t(7), C.c_int(7)
    assert L.cvo_fe_pixel_layout(K.GREY8, 64, 64, None, C.byref(rows)) != 0
    assert L.cvo_fe_pixel_layout(K.GREY8, 64, 64, C.byref(row), None) != 0
    assert L.cvo_fe_pixel_layout(K.YUY2, 65, 64, C.byref(row), C.byref(rows)) != 0 and (row.value, rows.value) == (7, 7)
    assert L.cvo_fe_set_pixel_format(None, K.GREY8) != 0 and L.cvo_fe_get_pixel_format(None, C.byref(rows)) != 0
    u8 = (C.c_uint8 * 16)()
    p = C.cast(u8, C.POINTER(C.c_uint8))
    for args in ((None, 4, 2, 2, K.GREY8, p), (p, 4, 2, 2, K.GREY8, None), (p, 1, 2, 2, K.GREY8, p), (p, 4, 0, 2, K.GREY8, p),
                 (p, 8193, 8193, 1, K.GREY8, p), (p, 4, 2, 8193, K.GREY8, p), (p, 4, 2, 2, 12, p), (p, 4, 2, 2, -1, p),
                 (p, 4, 1, 2, K.YUY2, p), (p, 4, 2, 1, K.NV12, p), (p, 4, 1, 2, K.BAYER_RGGB8, p), (p, 5, 2, 2, K.BGR8, p)):
        assert L.cvo_fe_unpack_image(0, *args) == -1, args     # (CVO_HIP_ERR_INVALID, before any device is asked for)


def test_bgr8_is_a_copy_on_the_host(pkg):
    """under BGR8 the stand-alone entry is a copy: no device is asked for"""
    F = pkg.frontend
    for w, h, stride in ((1, 1, None), (5, 3, None), (5, 3, 22), (64, 2, 200)):
        rows, row = K.layout(K.BGR8, w, h)
        pitch = row if stride is None else stride
        src = np.random.default_rng(w).integers(0, 256, (rows, pitch), dtype=np.uint8)
        keep = src.copy()
        got = F.unpack_image(src, K.BGR8, w, h, stride=stride)
        assert np.array_equal(got, K.unpack(src[:, :row], K.BGR8, w, h)) and np.array_equal(src, keep)


def test_the_anchors_and_the_grey_axis():
    y = np.arange(256)
    grey = K.bt601(y, np.full(256, 128), np.full(256, 128))
    assert grey[16].tolist() == [0, 0, 0] and grey[235].tolist() == [255, 255, 255]
    assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all()
    assert (np.diff(grey[:, 0].astype(int)) >= 0).all() and grey[0].tolist() == [0, 0, 0] and grey[255].tolist() == [255, 255, 255]
    k = (np.array([255 / 219, 1.402 * 255 / 224, 1.772 * (0.114 / 0.587) * 255 / 224, 1.402 * (0.299 / 0.587) * 255 / 224,
                   1.772 * 255 / 224]) * 2 ** 20)
    assert np.rint(k).astype(int).tolist() == [1220945, 1673555, 410793, 852458, 2115221]


def test_the_accumulators_fit_int32_over_all_triples():
    y, u, v = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    worst = max(int(np.abs(a).max()) for a in K.accumulators(y.ravel(), u.ravel(), v.ravel()))
    assert worst == 560963210 < 2 ** 31


def test_y_below_16_is_not_clamped():
    """(0, 128, 255): with Y clamped the red channel would be 16 levels higher"""
    assert K.bt601(np.array([0]), np.array([128]), np.array([255]))[0].tolist() != M.y_clamped(
        np.array([[0, 128, 0, 255]], np.uint8), K.YUY2, 2, 1)[0, 0].tolist()


@pytest.mark.parametrize("fmt", K.BAYER, ids=[K.NAMES[f] for f in K.BAYER])
def test_flat_colours_and_ramps_through_the_demosaic(fmt):
    for w, h in ((2, 2), (3, 2), (5, 7), (13, 9)):
        flat = np.empty((h, w, 3), np.uint8)
        flat[:] = (10, 200, 77)
        assert np.array_equal(K.unpack(K.mosaic(flat, fmt), fmt, w, h), flat), (w, h)
    y, x = np.mgrid[0:9, 0:13]
    ramp = np.stack([x + 2 * y, 3 * x + y + 5, 100 - x - y], -1).astype(np.uint8)
    got = K.unpack(K.mosaic(ramp, fmt), fmt, 13, 9)
    assert np.array_equal(got[1:-1, 1:-1], ramp[1:-1, 1:-1]) and not np.array_equal(got, ramp)
    # the letters: (0,0) (1,0) / (0,1) (1,1)
    letters = K.NAMES[fmt][6:10]
    one = np.zeros((2, 2, 3), np.uint8)
    one[:, :] = (1, 2, 3)                                     # B G R
    assert "".join("BGR"[c - 1] for c in K.mosaic(one, fmt).ravel()) == letters
    # a tiling that loses nothing is the restatement
    src = K.make_input(fmt, 130, 34, "random")
    assert np.array_equal(M._tiled(src, fmt, 130, 34, False, False), K.unpack(src, fmt, 130, 34))


def test_the_sizes_and_the_inputs_of_the_gpu_test():
    assert set(K.SIZES) == {(1, 1), (2, 1), (2, 2), (4, 2), (6, 4), (10, 6), (13, 7), (66, 18), (130, 34), (64, 64), (8192, 2), (2, 8192)}
    for fmt in K.FORMATS:
        sizes = K.sizes_for(fmt)
        smallest = (2, 2) if fmt in K.BAYER or fmt == K.NV12 else (2, 1) if fmt in K.YUV else (1, 1)
        assert sizes[0] == smallest and {(4, 2), (6, 4), (10, 6), (66, 18), (130, 34), (64, 64), (8192, 2), (2, 8192)} <= set(sizes)
        assert ((13, 7) in sizes) == (fmt not in K.YUV)
        for w, h, kind in K.cases(fmt):
            a, b = K.make_input(fmt, w, h, kind), K.make_input(fmt, w, h, kind)
            assert a.shape == K.layout(fmt, w, h) and a.dtype == np.uint8 and np.array_equal(a, b)
    assert 10 % 4 == 2 and 66 % 4 and 130 % 4 and 66 > 64 and 18 > 16 and 130 > 128 and 34 > 32
    kinds = K.kinds_for(K.BAYER_GRBG8, 130, 34)
    assert {"corner-%d" % k for k in range(4)} | {"seam-%d" % k for k in range(4)} <= set(kinds)
    assert {(x & 1, y & 1) for x, y in K.IMPULSES["corner"]} == {(x & 1, y & 1) for x, y in K.IMPULSES["seam"]} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert not any(k.startswith("seam") for k in K.kinds_for(K.BAYER_GRBG8, 10, 6))


@pytest.mark.parametrize("fmt", K.YUV, ids=[K.NAMES[f] for f in K.YUV])
def test_the_moderate_input_shows_the_arithmetic_and_random_bytes_saturate(fmt):
    """at most 10 % of the moderate input's pixels have a channel at 0 or 255; uniform random bytes saturate about
    85 % (asserted: between 75 % and 95 %), so they count as the saturation input only"""
    w, h = 64, 64
    src = K.make_input(fmt, w, h, "moderate")
    y, u, v = K.yuv_planes(src, fmt, w, h)
    assert 48 <= y.min() and y.max() <= 208 and 96 <= min(u.min(), v.min()) and max(u.max(), v.max()) <= 160
    moderate, random = K.saturated(K.unpack(src, fmt, w, h)), K.saturated(K.unpack(K.make_input(fmt, w, h, "random"), fmt, w, h))
    print(K.NAMES[fmt], "saturated: moderate %.3f random %.3f" % (moderate, random))
    assert moderate <= 0.10 and 0.75 <= random <= 0.95


@pytest.mark.parametrize("mutant", M.MUTANTS, ids=[m[0] for m in M.MUTANTS])
def test_an_input_of_the_gpu_test_tells_the_mutant_from_the_restatement(mutant):
    """for every format the mutant applies to, at least one (size, input) of the GPU test differs"""
    name, formats, wrong = mutant
    assert formats
    for fmt in formats:
        told = []
        for w, h, kind in K.cases(fmt):
            if w * h > 130 * 34:
                continue                                      # (the small sizes suffice, and keep this test quick)
            src = K.make_input(fmt, w, h, kind)
            if not np.array_equal(wrong(src, fmt, w, h), K.unpack(src, fmt, w, h)):
                told.append((w, h, kind))
        print(name, K.NAMES[fmt], "told by", len(told), "inputs, first", told[:1])
        assert told, (name, K.NAMES[fmt])
