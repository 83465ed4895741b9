"""The cases on which the selector's depth mode (the selection contract of include/cvo_frontend.h) is held to
tests/selector_depth_ref.py: frames of selector_ref_cases.py at the sizes with partial blocks and threshold cells past
the end, each under every hole pattern and every budget.  No test lives here.

A hole pattern is a validity plane made from the frame's own planes and thresholds, so that the holes lie where the
selector looks.  They are data, chosen until the census of tests/test_selector_depth_cpu.py held."""
import numpy as np

import selector_depth_ref as dr
import selector_ref_cases as sc

FRAMES = tuple(c for c in sc.CASES if c.name in (
    "tex1_s2_96x64", "stripes_s0_96x64", "noise_s4_96x64",
    "tex6_s7_65x67", "stripes_s0_65x67",
    "tex1_s14_65x70", "tex6_s15_65x70",
    "tex1_s9_127x193", "stripes_s0_127x193"))
SIZES = ((96, 64), (65, 67), (65, 70), (127, 193))

PATTERNS = ("none", "all", "winner", "level0_gone", "level01_gone", "checkerboard", "columns", "half", "blobs30",
            "blobs90", "few")


def budgets(w, h):
    return (1, 50, w * h // 8, 10 ** 6)


def _blobs(w, h, seed, share):
    """seeded random blobs covering about `share` of the image: squares of 3 to 9 pixels, a few at a time (one per
    2000 pixels of the image) until the share is reached"""
    rng = np.random.default_rng(seed)
    hole = np.zeros((h, w), bool)
    while hole.mean() < share:
        for _ in range(max(1, w * h // 2000)):
            s = int(rng.integers(3, 10))
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            hole[y:y + s, x:x + s] = True
    return hole


def hole_pattern(name, ag0, ag1, ag2, ths_smoothed, seed=0):
    """-> valid, (h, w) bool"""
    h, w = ag0.shape
    ys, xs = np.mgrid[0:h, 0:w]
    full = np.ones((h, w), bool)
    if name == "none":
        return full
    if name == "all":
        return ~full
    if name == "winner":        # every pixel the unmasked first pass picked
        return dr.select_closed(ag0, ag1, ag2, ths_smoothed, 3, full)[0] == 0
    if name in ("level0_gone", "level01_gone"):
        th0, th1, _ = dr._cell_thresholds(ths_smoothed, w, h)
        hole = ag0 > th0
        if name == "level01_gone":
            hole = hole | (dr._level_planes(ag1, ag2, w, h)[0] > th1)
        return ~hole
    if name == "checkerboard":
        return (xs + ys) % 2 == 0
    if name == "columns":       # holes one pixel wide, every third column
        return xs % 3 != 1
    if name == "half":
        return xs >= w // 2
    if name == "blobs30":
        return ~_blobs(w, h, 1000 + seed, 0.30)
    if name == "blobs90":
        return ~_blobs(w, h, 2000 + seed, 0.90)
    if name == "few":           # valid on a few dozen pixels only: short runs along five rows inside the margin
        valid = ~full
        rng = np.random.default_rng(3000 + seed)
        for _ in range(12):
            y, x = int(rng.integers(6, h - 6)), int(rng.integers(6, w - 12))
            valid[y, x:x + 4] = True
        return valid
    raise ValueError(name)


def depth_of(valid):
    """a depth image with the holes of `valid`: values that differ from pixel to pixel, 0 where not valid"""
    h, w = valid.shape
    ys, xs = np.mgrid[0:h, 0:w]
    return np.where(valid, 2000 + (xs * 37 + ys * 101) % 6000, 0).astype(np.uint16)
