"""The cases on which the pixel selector is held to the reference's own code (test_selector_ref_cpu.py,
test_gpu_selector_ref.py, tools/make_golden.py), and the census that shows what they reach.  No test lives here.

A case is a frame at a size; every case runs at every budget (num_want) of its list.  Groups:
  raw      w % 32 <= 5 and h % 32 <= 3: the margin keeps every threshold read inside the cells makeHists wrote, so the
           reference is compared as it stands (define_unwritten off)
  defined  the other sizes: the reference reads cells it never wrote; compared with those cells defined as the last
           cell (oracle/ref_selector_harness.cpp).  Nothing is asserted about the reference with them undefined.
  large    a VGA and a 720p frame, for the compiled reference only (720p is of the defined kind)
"""
import ctypes
from collections import namedtuple

import numpy as np

f32 = np.float32

Case = namedtuple("Case", "name kind seed w h group budgets")

PY_MAX_PIXELS = 25000   # tests/selector_ref.py runs on cases up to this size


def _budgets(w, h):
    return (1, 7, 50, 400, w * h // 8, w * h, 10 ** 6)


def _case(kind, seed, w, h, group):
    return Case("%s_s%d_%dx%d" % (kind, seed, w, h), kind, seed, w, h, group, _budgets(w, h))


CASES = (
    # raw group
    [_case(k, s, 96, 64, "raw") for k, s in (("tex0.3", 1), ("tex1", 2), ("tex6", 3), ("noise", 4), ("flat", 0),
                                             ("steps", 0), ("stripes", 0))] +
    [_case(k, s, 128, 192, "raw") for k, s in (("tex1", 5), ("lowtex", 6), ("stripes", 0))] +
    [_case(k, s, 65, 67, "raw") for k, s in (("tex6", 7), ("stripes", 0))] +
    [_case(k, s, 644, 483, "raw") for k, s in (("tex1", 8), ("lowtex", 6))] +
    # defined group
    [_case(k, s, 127, 193, "defined") for k, s in (("tex1", 9), ("noise", 10), ("stripes", 0))] +
    [_case(k, s, 333, 251, "defined") for k, s in (("tex0.3", 11), ("tex6", 12))] +
    [_case(k, s, 352, 300, "defined") for k, s in (("tex1", 13), ("stripes", 0))] +
    [_case(k, s, 65, 70, "defined") for k, s in (("tex1", 14), ("steps", 0), ("tex6", 15))] +
    # large frames
    [_case("tex1", 16, 640, 480, "large"), _case("tex1", 17, 1280, 720, "large"), _case("quads", 0, 1280, 720, "large")]
)

DEFINED_SIZES = ((127, 193), (333, 251), (352, 300), (65, 70))


def reads_unwritten(w, h):
    """Does the selector read a threshold cell past the (w/32)*(h/32) it wrote?  xf <= w-6 and yf <= h-4 are visited."""
    return w % 32 > 5 or h % 32 > 3


def define_unwritten(case):
    return reads_unwritten(case.w, case.h)


def runs_in_python(case):
    return case.w * case.h <= PY_MAX_PIXELS


def on_gpu(case):
    """The GPU file's cases: everything up to 352x300, the VGA frame, and the one frame that reaches charTH == 0"""
    return case.w * case.h <= 352 * 300 or (case.w, case.h) == (640, 480) or case.kind == "quads"


STEP14_X, STEP15_X = 24, 44   # the columns left of frame "steps"' two steps


def frame(pkg, case):
    """(bgr h x w x 3 uint8, depth h x w uint16) of a case"""
    w, h = case.w, case.h
    dep = np.full((h, w), 5000, np.uint16)
    if case.kind.startswith("tex"):
        return pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=case.seed, texture=float(case.kind[3:]))
    if case.kind == "lowtex":
        from conftest import low_texture_frame
        return low_texture_frame(pkg, seed=case.seed, width=w, height=h)
    if case.kind == "noise":
        g = np.random.default_rng(case.seed).integers(0, 256, (h, w), dtype=np.uint8)
    elif case.kind == "flat":
        g = np.full((h, w), 90, np.uint8)
    elif case.kind == "steps":
        # built frame A (strict '>'): flat grey, so every cell's smoothed threshold is exactly 49; a vertical step of 14
        # grey levels (ag0 = 7^2 = 49 on both sides of it: NOT above the threshold) and one of 15 (7.5^2 = 56.25: above)
        g = np.full((h, w), 60, np.uint8)
        g[:, STEP14_X + 1:] += 14
        g[:, STEP15_X + 1:] += 15
    elif case.kind == "stripes":
        # built frame B (ties): periodic stripes, so that the pixels of a block hold bit-equal gradients; a slow ramp
        # down the image keeps the rows from being all alike
        y, x = np.mgrid[0:h, 0:w]
        g = (70 + 50 * ((x // 3) % 2) + 30 * ((y // 5) % 2) + 2 * (y // 16)).astype(np.uint8)
    elif case.kind == "quads":
        # built frame C (sub-sampling with charTH == 0, i.e. 255*num_want/numHave < 1 in the FINAL pass).  That takes a
        # second pass that keeps more than 255 pixels although the first kept few enough to ask for a large potential;
        # since a pass at a larger potential keeps at most 4 pixels where pass 1 kept one (around a corner of its grid),
        # no frame much below a megapixel gets there: hence 1280x720.
        # 72 clusters of 2x2 pixels 14 grey levels above a flat image (thresholds 49; a cluster pixel has ag0 = 98, the
        # ring around it 49: not above; odd origins keep levels 1 and 2 below their thresholds), each around a corner
        # (32k, 32l) of the grid of potential 32, inside ONE 3x3 block of potential 3 (k, l = 1 mod 3) and no two in one
        # block of potential 32.  Pass 1 keeps 72; num_want 1 then asks for potential int(sqrt(72*16) - 1) = 32, whose
        # four blocks around a corner keep one cluster pixel each: 288, and 255/288 < 1.
        assert (w, h) == (1280, 720)
        g = np.full((h, w), 60, np.uint8)
        corners = [(k, l) for l in range(1, 22, 3) for k in range(1, 40, 3)][:72]
        for k, l in corners:
            g[32 * l - 1:32 * l + 1, 32 * k - 1:32 * k + 1] += 14
    else:
        raise ValueError(case.kind)
    return np.repeat(g[:, :, None], 3, axis=2), dep   # (equal channels: the grey value is g itself)


def libc_pattern(n):
    """srand(3141592); rand() & 0xFF per pixel (ref thirdparty/PixelSelector2.cpp:36-38), from the C library itself"""
    libc = ctypes.CDLL(None)
    libc.srand(3141592)
    rand = libc.rand
    return bytes(rand() & 0xFF for _ in range(n))


def level_index(v, scale, add):
    return int(f32(v) * f32(scale) + f32(add))


CENSUS_KEYS = ("pot_1", "pot_2", "pot_3", "pot_4_7", "pot_ge_8", "pot_block_exceeds_image",
               "reselect_to_larger_pot", "reselect_to_smaller_pot", "no_reselect",
               "subsample_charth_0", "subsample_charth_pos", "subsample_off",
               "level_1_picks", "level_2_picks", "level_4_picks",
               "pick_in_block_cut_right", "pick_in_block_cut_bottom",
               "b2_tie_by_order", "b3_tie_by_order", "b4_tie_by_order",
               "pick_cell_past_end", "pick_column_aliased")

TIE_WORK_LIMIT = 3000000   # picks x block area up to which the ties of a run are counted


def census_add(census, case, budget, res, num_have, planes=None, ths_smoothed=None, pre_map=None):
    """Adds one run to `census` (a dict of counts over CENSUS_KEYS).  res: the truth's pot_used and reselected; num_have:
    what its final selection pass kept before any sub-sampling; pre_map (with the planes and the smoothed thresholds,
    for the runs whose picks are looked at): that pass's map."""
    for k in CENSUS_KEYS:
        census.setdefault(k, 0)
    w, h, pot = case.w, case.h, res["pot_used"]
    census["pot_1" if pot == 1 else "pot_2" if pot == 2 else "pot_3" if pot == 3 else
           "pot_4_7" if pot <= 7 else "pot_ge_8"] += 1
    if 4 * pot > max(w, h):
        census["pot_block_exceeds_image"] += 1
    census["no_reselect" if not res["reselected"] else
           "reselect_to_larger_pot" if pot > 3 else "reselect_to_smaller_pot"] += 1
    with np.errstate(divide="ignore"):
        quotia = f32(budget) / f32(num_have)
    if float(quotia) < 0.95:
        census["subsample_charth_0" if int(f32(255) * quotia) == 0 else "subsample_charth_pos"] += 1
    else:
        census["subsample_off"] += 1
    if pre_map is None:
        return
    assert np.count_nonzero(pre_map) == num_have
    ys, xs = np.nonzero(pre_map)
    lv = pre_map[ys, xs]
    for level, key in ((1, "level_1_picks"), (2, "level_2_picks"), (4, "level_4_picks")):
        census[key] += int((lv == level).sum())
    w32, ncell = w // 32, (w // 32) * (h // 32)
    side = (lv * pot).astype(np.int64)           # of the block that chose the pick: pot, 2 pot, 4 pot
    census["pick_in_block_cut_right"] += int(((xs // side) * side + side > w).sum())
    census["pick_in_block_cut_bottom"] += int(((ys // side) * side + side > h).sum())
    census["pick_cell_past_end"] += int((((xs >> 5) + (ys >> 5) * w32) >= ncell).sum())
    census["pick_column_aliased"] += int(((xs >> 5) == w32).sum())
    if len(xs) == 0 or int((side * side).sum()) > TIE_WORK_LIMIT:
        return
    # ties: another pixel of the pick's block, inside the margin and above ITS threshold, holds the pick's value bit for bit
    ths = ths_smoothed.ravel()
    a0, a1, a2 = planes
    i1x = [level_index(x, 0.5, 0.25) for x in range(w)]
    i1y = [level_index(y, 0.5, 0.25) for y in range(h)]
    i2x = [level_index(x, 0.25, 0.125) for x in range(w)]
    i2y = [level_index(y, 0.25, 0.125) for y in range(h)]
    dw1 = f32(0.75)
    dw2 = dw1 * dw1

    def value_and_threshold(x, y, level):
        th0 = ths[min((x >> 5) + (y >> 5) * w32, ncell - 1)]
        if level == 1:
            return a0[y, x], th0
        if level == 2:
            return a1[i1y[y], i1x[x]], th0 * dw1
        return a2[i2y[y], i2x[x]], (th0 * dw1) * dw2

    for x, y, level, s in zip(xs.tolist(), ys.tolist(), lv.astype(int).tolist(), side.tolist()):
        v, _ = value_and_threshold(x, y, level)
        x0, y0 = x // s * s, y // s * s
        tie = False
        for yy in range(max(y0, 4), min(y0 + s, h - 3)):          # yf > h-4 is skipped
            for xx in range(max(x0, 4), min(x0 + s, w - 5)):      # xf >= w-5 is skipped
                if (xx, yy) == (x, y):
                    continue
                vv, th = value_and_threshold(xx, yy, level)
                if vv == v and vv > th:
                    tie = True
                    break
            if tie:
                break
        if tie:
            census[{1: "b2_tie_by_order", 2: "b3_tie_by_order", 4: "b4_tie_by_order"}[level]] += 1
