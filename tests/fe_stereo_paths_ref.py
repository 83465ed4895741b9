"""A numpy restatement of step 4 of the stereo contract (include/cvo_frontend.h, at cvo_fe_stereo) under a path mask
(cvo_fe_set_stereo_paths): eight directions r = (rx, ry), bit b of the mask choosing direction b, S the sum of L_r over
the chosen ones.  Every other step is tests/fe_stereo_ref.py's, fed with the masked S.  Two forms of the sums: a
vectorised one, row by row with the previous row shifted by rx, and a loop over pixels that follows the contract's
sentence literally ("a pixel whose p - r lies outside the image is the first pixel of its path").  Also here: the one
case the diagonals add, `tall`, and a frame under a stereo rig with a mask."""
import numpy as np

import fe_stereo_ref as S

PATHS_4, PATHS_8 = 0x0F, 0xFF
# bit -> (rx, ry)
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1))


def bits(mask):
    assert 1 <= mask <= 0xFF
    return [b for b in range(8) if mask >> b & 1]


def _step(prev, Crow, p1, p2):
    """one step of the recurrence for a row of pixels: prev and Crow are n x D"""
    m = prev.min(axis=1, keepdims=True)
    below = np.full_like(prev, S.BIG)
    below[:, 1:] = prev[:, :-1] + p1
    above = np.full_like(prev, S.BIG)
    above[:, :-1] = prev[:, 1:] + p1
    return Crow + np.minimum(np.minimum(prev, m + p2), np.minimum(below, above)) - m


def direction(C, p1, p2, rx, ry):
    """L_r of one direction, h x w x D int64: row by row, the previous row shifted by rx"""
    C = np.asarray(C, np.int64)
    h, w, D = C.shape
    if ry == 0:                                            # along a row: the existing scan, steps over x
        Ct = C.transpose(1, 0, 2)
        if rx > 0:
            return S._scan(Ct, p1, p2).transpose(1, 0, 2)
        return S._scan(Ct[::-1], p1, p2)[::-1].transpose(1, 0, 2)
    L = np.empty_like(C)
    rows = range(h) if ry > 0 else range(h - 1, -1, -1)
    x = np.arange(w)
    inside = (x - rx >= 0) & (x - rx < w)                  # p - r has a column of the image
    last = None
    for y in rows:
        if last is None:
            L[y] = C[y]                                    # p - r has no row of the image
        else:
            prev = np.zeros((w, D), np.int64)
            prev[inside] = L[last][(x - rx)[inside]]
            L[y] = np.where(inside[:, None], _step(prev, C[y], p1, p2), C[y])
        last = y
    return L


def direction_loops(C, p1, p2, rx, ry):
    """L_r again, one pixel and one d at a time"""
    h, w, D = C.shape
    L = np.zeros((h, w, D), np.int64)
    ys = range(h) if ry >= 0 else range(h - 1, -1, -1)
    xs = range(w) if rx >= 0 else range(w - 1, -1, -1)
    for y in ys:
        for x in xs:
            py, px = y - ry, x - rx
            if not (0 <= py < h and 0 <= px < w):
                L[y, x] = C[y, x]
                continue
            prev = [int(v) for v in L[py, px]]
            m = min(prev)
            for d in range(D):
                terms = [prev[d], m + p2]
                if d - 1 >= 0:
                    terms.append(prev[d - 1] + p1)
                if d + 1 < D:
                    terms.append(prev[d + 1] + p1)
                L[y, x, d] = int(C[y, x, d]) + min(terms) - m
    return L


def path_sums(C, p1, p2, mask, one=direction):
    """4 under a mask: S h x w x D uint16.  (`one` puts another form of a direction in its place: the loop form, the
    mutants of tests/fe_stereo_paths_mutants.py.)"""
    Sv = np.zeros(C.shape, np.int64)
    for b in bits(mask):
        Sv += one(C, p1, p2, *DIRS[b])
    assert Sv.max() <= len(bits(mask)) * (64 + 255)
    return Sv.astype(np.uint16)


def path_sums_loops(C, p1, p2, mask):
    return path_sums(C, p1, p2, mask, one=direction_loops)


def volume(left, right, D):
    """(grey, census and C of a pair)"""
    gl, gr = S.grey(left), S.grey(right)
    cl, cr = S.census(gl), S.census(gr)
    return dict(gray_l=gl, gray_r=gr, census_l=cl, census_r=cr), S.cost(cl, cr, D)


def match(left, right, st, fx, depth_scale, mask):
    """fe_stereo_ref.match() under a path mask: every plane of a stereo frame, by name"""
    pre, C = volume(left, right, st["max_disp"])
    Sv = path_sums(C, st["p1"], st["p2"], mask)
    return dict(S.decide(Sv, st, fx, depth_scale), **pre)


def rig_frame(RG, rig, raw_l, raw_r, st, mask):
    """fe_stereo_rig_ref.frame() (RG: that module) under a path mask: the lines around the masked S, restated"""
    import fe_rectify_ref as R
    h, w = raw_l.shape[:2]
    (qul, qvl), (qur, qvr) = RG.rig_map(rig, 0, w, h), RG.rig_map(rig, 1, w, h)
    rect_l, rect_r = R.remap_colour(raw_l, qul, qvl), R.remap_colour(raw_r, qur, qvr)
    VL, VR = RG.valid(qul, qvl), RG.valid(qur, qvr)
    P = match(rect_l, rect_r, dict(st, baseline=rig["baseline"]), rig["fx"], rig["depth_scale"], mask)
    xr = np.arange(w)[None, :] - P["dL"]
    out = ~VL | ((xr >= 0) & ~VR[np.arange(h)[:, None], np.clip(xr, 0, w - 1)])
    flags = (P["flags"] | np.where(out, RG.OUTSIDE, 0)).astype(np.uint8)
    keep = flags == 0
    return dict(P, flags_before=P["flags"], flags=flags, disparity=np.where(keep, P["disparity"], 0).astype(np.uint16),
                depth=np.where(keep, P["depth"], 0).astype(np.uint16), rect_l=rect_l, rect_r=rect_r,
                valid=(VL.astype(np.uint8) | (VR.astype(np.uint8) << 1)))


# ---- the cases --------------------------------------------------------------------------------------
# `tall`: 64 wide and 321 high, so that a wrapped line (one column index, h steps, the column moving by rx per step and
# wrapping round the image) wraps five times; 321 = 8 * 40 + 1 leaves one step for the last chunk of eight.  The
# transposed situation, for one wave per true diagonal, is fe_stereo_ref's `wide` (1241 x 64).
# name: (width, height, settings, scene) as fe_stereo_ref.EDGE_CASES
PATH_CASES = {
    "tall": (64, 321, S.make_stereo(max_disp=32), ("pair", 86, 15.0, 6.0, S.PAD)),
}


def inputs(name):
    """(width, height, settings, left, right) of a case by name: a PATH_CASES entry, else an EDGE_CASES one, else a
    CASES one"""
    if name in PATH_CASES:
        w, h, st, scene = PATH_CASES[name]
        left, right, _ = S.pair(w, h, *scene[1:4], pad=scene[4])
        return w, h, st, left, right
    if name in S.EDGE_CASES:
        st, left, right, _ = S.edge_inputs(name)
        return S.EDGE_CASES[name][:2] + (st, left, right)
    st, left, right, _ = S.case_inputs(name)
    return S.CASES[name][:2] + (st, left, right)


_VOL = {}
_DONE = {}


def case_volume(name):
    """(the planes in front of C, C, settings) of a case, computed once and left unchanged"""
    if name not in _VOL:
        _, _, st, left, right = inputs(name)
        pre, C = volume(left, right, st["max_disp"])
        for a in tuple(pre.values()) + (C,):
            a.setflags(write=False)
        _VOL[name] = (pre, C, st)
    return _VOL[name]


def case_planes(name, mask):
    """match() of a case under a mask, computed once and left unchanged"""
    key = (name, mask)
    if key not in _DONE:
        pre, C, st = case_volume(name)
        out = dict(S.decide(path_sums(C, st["p1"], st["p2"], mask), st, S.FX, S.SCALE), **pre)
        for a in out.values():
            a.setflags(write=False)
        _DONE[key] = out
    return _DONE[key]
