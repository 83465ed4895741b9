"""The selection contract of include/cvo_frontend.h (CVO_FE_SELECT_DEPTH: a pixel without depth does not compete)
restated twice.  The two statements of `select` share no code:

  select_walk    the reference's walk (ref thirdparty/PixelSelector2.cpp:290-433; the shape of selector_ref.select):
                 B4s, their B3s, their B2s, rows, columns, three running maxima and two sticky "-2" marks; a pixel that
                 is not valid leaves where a pixel outside the margin leaves.
  select_closed  the three rules in the comment above k_fe_select, vectorised: per B2, B3 and B4 the first largest
                 among the VALID pixels inside the margin above the level's threshold, a B3 only without a level-0
                 candidate, a B4 only without a candidate of level 0 or 1.

Around them: make_hists (vectorised; the thresholds read every pixel), make_maps(..., valid) (makeMaps on the counts
select gives, numHave == 0 included), topup (the Canny top-up's last step on an edge plane) and cloud (back-projection
and the raw colour features).  It reads nothing of oracle/ and nothing of the product.

`valid` is a (h, w) bool plane: Z != 0.  Arithmetic as in selector_ref.py: what the reference forms in float is
formed in np.float32.

`mutant=`: one deliberate misreading each (MUTANTS), carried by the closed form, the thresholds and the top-up;
tests/test_selector_depth_cpu.py names the case that tells each from the contract.
"""
import numpy as np

f32 = np.float32

MUTANTS = (
    "valid_level0_only",     # validity tested for level 0 only: a hole still competes at levels 1 and 2
    "valid_after_select",    # validity applied after selection: the default mode's map with the holes removed
    "invalid_sets_marks",    # a hole above a threshold is no candidate but still marks its B3 / B4
    "valid_at_level_pixel",  # validity looked up at the level's own pixel (2(x/2), 2(y/2)), (4(x/4), 4(y/4))
    "ths_valid_only",        # the cell histograms over valid pixels only
    "topup_ignores_depth",   # the top-up takes the first free edge pixel, valid or not
)


# ---- thresholds ---------------------------------------------------------------------------------------------------

def make_hists(ag0, valid=None, mutant=None):
    """makeHists (ref :71-136) -> (ths, thsSmoothed); every pixel counts, valid or not (contract 1)"""
    ag0 = np.ascontiguousarray(ag0, f32)
    h, w = ag0.shape
    w32, h32 = w // 32, h // 32
    g = np.minimum(np.sqrt(ag0).astype(np.int64), 48)
    ys, xs = np.mgrid[0:h, 0:w]
    counted = (xs >= 1) & (ys >= 1) & (xs <= w - 2) & (ys <= h - 2) & (xs < 32 * w32) & (ys < 32 * h32)
    if mutant == "ths_valid_only":
        counted &= valid
    ths = np.zeros((h32, w32), f32)
    for cy in range(h32):
        for cx in range(w32):
            sel = counted[32 * cy:32 * cy + 32, 32 * cx:32 * cx + 32]
            bins = np.bincount(g[32 * cy:32 * cy + 32, 32 * cx:32 * cx + 32][sel], minlength=49)
            th = int(f32(int(sel.sum())) * f32(0.5) + f32(0.5))
            q = 90
            run = np.cumsum(bins)
            over = np.nonzero(run > th)[0]
            if len(over):
                q = int(over[0])
            ths[cy, cx] = f32(q + 7)
    sm = np.zeros((h32, w32), f32)
    for y in range(h32):
        for x in range(w32):
            s, num = f32(0), f32(0)
            # the reference's order of the nine terms (float sums of small integers: any order gives the same bits,
            # kept all the same)
            for dx, dys in ((-1, (-1, 1, 0)), (1, (-1, 1, 0)), (0, (-1, 1, 0))):
                for dy in dys:
                    if 0 <= x + dx < w32 and 0 <= y + dy < h32:
                        num += f32(1)
                        s += ths[y + dy, x + dx]
            sm[y, x] = (s / num) * (s / num)
    return ths, sm


def _cell_thresholds(sm, w, h):
    """per pixel th0, th1, th2 (float32 planes): the cell past the end reads the last cell"""
    w32, ncell = w // 32, (w // 32) * (h // 32)
    ys, xs = np.mgrid[0:h, 0:w]
    cell = np.minimum((xs >> 5) + (ys >> 5) * w32, ncell - 1)
    th0 = np.ascontiguousarray(sm, f32).ravel()[cell]
    dw1 = f32(0.75)
    dw2 = dw1 * dw1
    th1 = th0 * dw1
    th2 = th1 * dw2
    return th0, th1, th2


def _level_planes(ag1, ag2, w, h):
    """ag1 and ag2 as the level-0 pixel (xf, yf) looks them up (ref :343, :355)"""
    i1x = (np.arange(w, dtype=f32) * f32(0.5) + f32(0.25)).astype(np.int64)
    i1y = (np.arange(h, dtype=f32) * f32(0.5) + f32(0.25)).astype(np.int64)
    i2x = (np.arange(w, dtype=f32) * f32(0.25) + f32(0.125)).astype(np.int64)
    i2y = (np.arange(h, dtype=f32) * f32(0.25) + f32(0.125)).astype(np.int64)
    # (pixels outside the margin may index past a plane's end; they are never candidates: clipped)
    h1, w1 = ag1.shape
    h2, w2 = ag2.shape
    a1 = ag1[np.minimum(i1y, h1 - 1)[:, None], np.minimum(i1x, w1 - 1)[None, :]]
    a2 = ag2[np.minimum(i2y, h2 - 1)[:, None], np.minimum(i2x, w2 - 1)[None, :]]
    return a1, a2


# ---- select, the closed form --------------------------------------------------------------------------------------

def _in_visiting_order(a, pot, fill):
    """a (h, w) plane as (number of B4s, 16 pot^2): each B4's pixels in the reference's visiting order -- B3s, their
    B2s, rows, columns -- the image padded with `fill` to whole B4s"""
    h, w = a.shape
    side = 4 * pot
    H, W = -(-h // side) * side, -(-w // side) * side
    full = np.full((H, W), fill, a.dtype)
    full[:h, :w] = a
    # axes: B4 row, B3 row, B2 row, y1, B4 column, B3 column, B2 column, x1
    full = full.reshape(H // side, 2, 2, pot, W // side, 2, 2, pot).transpose(0, 4, 1, 5, 2, 6, 3, 7)
    return full.reshape((H // side) * (W // side), 16 * pot * pot)


def _first_largest(value, cand, where, per_b4, keep=None):
    """per block (per_b4 of them in a B4: 16 B2s, 4 B3s, 1 B4) the first largest value among the candidates ->
    (flat pixel indices of the picks, which blocks hold a candidate at all); keep: the blocks that may pick"""
    n = value.shape[0]
    v = np.where(cand, value, np.float32(-1)).reshape(n * per_b4, -1)    # (every candidate is above a threshold >= 0)
    has = cand.reshape(n * per_b4, -1).any(axis=1)
    take = has if keep is None else has & keep
    first = v[take].argmax(axis=1)                                      # (argmax: the first of equals)
    return where.reshape(n * per_b4, -1)[take, first], has


def select_closed(ag0, ag1, ag2, ths_smoothed, pot, valid, mutant=None):
    """-> (map (h, w) float32, [n2, n3, n4])"""
    ag0, ag1, ag2 = (np.ascontiguousarray(a, f32) for a in (ag0, ag1, ag2))
    h, w = ag0.shape
    valid = np.ascontiguousarray(valid, bool)
    ys, xs = np.mgrid[0:h, 0:w]
    margin = (xs >= 4) & (xs < w - 5) & (ys >= 4) & (ys <= h - 4)
    th0, th1, th2 = _cell_thresholds(ths_smoothed, w, h)
    a1, a2 = _level_planes(ag1, ag2, w, h)
    v0 = v1 = v2 = valid
    if mutant in ("valid_level0_only", "valid_after_select"):
        v1 = v2 = np.ones_like(valid)
        if mutant == "valid_after_select":
            v0 = v1
    elif mutant == "valid_at_level_pixel":
        v1 = valid[(2 * (ys // 2)), (2 * (xs // 2))]
        v2 = valid[(4 * (ys // 4)), (4 * (xs // 4))]
    above0, above1, above2 = margin & (ag0 > th0), margin & (a1 > th1), margin & (a2 > th2)
    order = lambda a, fill: _in_visiting_order(a, pot, fill)
    c0, c1, c2 = order(above0 & v0, False), order(above1 & v1, False), order(above2 & v2, False)
    where = order(ys * w + xs, -1)
    n = c0.shape[0]
    # what marks a B3 (a level-0 candidate in it) and a B4 (a candidate of level 0, or of level 1 in a B3 without)
    m0, m1 = (order(above0, False), order(above1, False)) if mutant == "invalid_sets_marks" else (c0, c1)
    p2, _ = _first_largest(order(ag0, 0), c0, where, 16)
    b3_free = ~m0.reshape(n * 4, -1).any(axis=1)
    p3, _ = _first_largest(order(a1, 0), c1, where, 4, keep=b3_free)
    b4_free = ~(m0.any(axis=1) | (m1.reshape(n * 4, -1).any(axis=1) & b3_free).reshape(n, 4).any(axis=1))
    p4, _ = _first_largest(order(a2, 0), c2, where, 1, keep=b4_free)
    out = np.zeros(w * h, f32)
    out[p2], out[p3], out[p4] = 1.0, 2.0, 4.0
    out = out.reshape(h, w)
    if mutant == "valid_after_select":
        out[~valid] = 0.0
        return out, [int((out == 1).sum()), int((out == 2).sum()), int((out == 4).sum())]
    return out, [len(p2), len(p3), len(p4)]


# ---- select, the walk ---------------------------------------------------------------------------------------------

def select_walk(ag0, ag1, ag2, ths_smoothed, pot, valid):
    """-> (map (h, w) float32, [n2, n3, n4]): the reference's loops with `valid` in the margin's test"""
    h, w = ag0.shape
    w1, w2, w32 = w // 2, w // 4, w // 32
    ncell = (w // 32) * (h // 32)
    dw1 = f32(0.75)
    dw2 = dw1 * dw1
    cells = []
    for t in np.asarray(ths_smoothed, f32).ravel():
        t0 = f32(t)
        t1 = t0 * dw1
        t2 = t1 * dw2
        cells.append((float(t0), float(t1), float(t2)))
    a0s = np.asarray(ag0, f32).ravel().tolist()
    a1s = np.asarray(ag1, f32).ravel().tolist()
    a2s = np.asarray(ag2, f32).ravel().tolist()
    ok = np.asarray(valid, bool).ravel().tolist()
    out = [0.0] * (w * h)
    i1x = [int(f32(x) * f32(0.5) + f32(0.25)) for x in range(w)]
    i1y = [int(f32(y) * f32(0.5) + f32(0.25)) for y in range(h)]
    i2x = [int(f32(x) * f32(0.25) + f32(0.125)) for x in range(w)]
    i2y = [int(f32(y) * f32(0.25) + f32(0.125)) for y in range(h)]
    big = float(f32(1e10))
    n2 = n3 = n4 = 0
    for y4 in range(0, h, 4 * pot):
        for x4 in range(0, w, 4 * pot):
            my3, mx3 = min(4 * pot, h - y4), min(4 * pot, w - x4)
            best_idx4, best_val4 = -1, 0.0
            for y3 in range(0, my3, 2 * pot):
                for x3 in range(0, mx3, 2 * pot):
                    x34, y34 = x3 + x4, y3 + y4
                    my2, mx2 = min(2 * pot, h - y34), min(2 * pot, w - x34)
                    best_idx3, best_val3 = -1, 0.0
                    for y2 in range(0, my2, pot):
                        for x2 in range(0, mx2, pot):
                            x234, y234 = x2 + x34, y2 + y34
                            my1, mx1 = min(pot, h - y234), min(pot, w - x234)
                            best_idx2, best_val2 = -1, 0.0
                            for y1 in range(my1):
                                for x1 in range(mx1):
                                    xf, yf = x1 + x234, y1 + y234
                                    idx = xf + w * yf
                                    if xf < 4 or xf >= w - 5 or yf < 4 or yf > h - 4 or not ok[idx]:
                                        continue
                                    cell = (xf >> 5) + (yf >> 5) * w32
                                    th0, th1, th2 = cells[cell if cell < ncell else ncell - 1]
                                    a0 = a0s[idx]
                                    if a0 > th0 and a0 > best_val2:
                                        best_val2, best_idx2 = a0, idx
                                        best_idx3 = -2
                                        best_idx4 = -2
                                    if best_idx3 == -2:
                                        continue
                                    a1 = a1s[i1x[xf] + i1y[yf] * w1]
                                    if a1 > th1 and a1 > best_val3:
                                        best_val3, best_idx3 = a1, idx
                                        best_idx4 = -2
                                    if best_idx4 == -2:
                                        continue
                                    a2 = a2s[i2x[xf] + i2y[yf] * w2]
                                    if a2 > th2 and a2 > best_val4:
                                        best_val4, best_idx4 = a2, idx
                            if best_idx2 > 0:
                                out[best_idx2] = 1.0
                                best_val3 = big
                                n2 += 1
                    if best_idx3 > 0:
                        out[best_idx3] = 2.0
                        best_val4 = big
                        n3 += 1
            if best_idx4 > 0:
                out[best_idx4] = 4.0
                n4 += 1
    return np.array(out, f32).reshape(h, w), [n2, n3, n4]


# ---- makeMaps, the top-up, the cloud ------------------------------------------------------------------------------

def make_maps(ag0, ag1, ag2, num_want, pattern, valid, select=select_closed, mutant=None, memo=None):
    """makeHists + makeMaps (ref :137-286; contract 3) -> dict(map, count, pot_used, reselected, ths_smoothed, num_have,
    first_have, char_th).  With no pixel kept the float divisions are IEEE's, as k_fe_decide does them: quotia = +inf,
    the ideal potential int(sqrt(0) - 1) -> 1, a second pass at potential 1, no sub-sampling.  `memo`: a dict the
    caller keeps for ONE set of planes, validity, select and mutant: the passes do not depend on num_want."""
    ag0, ag1, ag2 = (np.ascontiguousarray(a, f32) for a in (ag0, ag1, ag2))
    h, w = ag0.shape
    memo = {} if memo is None else memo
    if "hists" not in memo:
        memo["hists"] = make_hists(ag0, valid, mutant)
    ths, sm = memo["hists"]
    kw = {} if select is select_walk else {"mutant": mutant}
    want = f32(num_want)
    pot, passes, first_have = 3, 0, None
    with np.errstate(divide="ignore", invalid="ignore"):
        while True:
            if pot not in memo:
                memo[pot] = select(ag0, ag1, ag2, sm, pot, valid, **kw)
            mp, n = memo[pot][0].copy(), memo[pot][1]
            passes += 1
            num_have = f32(n[0] + n[1] + n[2])
            if first_have is None:
                first_have = int(num_have)
            quotia = want / num_have
            if passes == 2:
                break
            ideal = int(np.sqrt(num_have * f32(pot + 1) * f32(pot + 1) / want) - f32(1))
            ideal = max(ideal, 1)
            if float(quotia) > 1.25 and pot > 1:
                pot = min(ideal, pot - 1)
            elif float(quotia) < 0.25:
                pot = max(ideal, pot + 1)
            else:
                break
    count, char_th = int(num_have), None
    if float(quotia) < 0.95:
        char_th = int(f32(255) * quotia) & 0xFF
        flat = mp.reshape(-1)
        chosen = np.flatnonzero(flat)
        drop = np.frombuffer(bytes(pattern[:len(chosen)]), np.uint8) > char_th
        flat[chosen[drop]] = 0.0
        count -= int(drop.sum())
    return {"map": mp, "count": count, "pot_used": pot, "reselected": passes - 1, "ths": ths, "ths_smoothed": sm,
            "num_have": int(num_have), "first_have": first_have, "char_th": char_th}


def topup_due(count, num_want):
    """ref src/pcd_generator.cpp:141-144; the count is of pixels with depth (contract 4)"""
    return count < int(num_want) // 3


def topup(mp, edges, valid, mutant=None):
    """contract 4: per 8x8 block the first pixel in row order that is an edge, free in the map and valid ->
    (the map with those pixels at 1, their number, the blocks whose first free edge pixel was a hole and that took a
    later one)"""
    out = np.array(mp, f32)
    h, w = out.shape
    edge = np.asarray(edges) != 0
    added = passed_a_hole = 0
    for y0 in range(0, h, 8):
        for x0 in range(0, w, 8):
            free = edge[y0:y0 + 8, x0:x0 + 8] & (out[y0:y0 + 8, x0:x0 + 8] == 0)
            ok = free if mutant == "topup_ignores_depth" else free & valid[y0:y0 + 8, x0:x0 + 8]
            hit = np.flatnonzero(ok.ravel())     # (row order inside the block)
            if len(hit) == 0:
                continue
            bw = ok.shape[1]
            out[y0 + hit[0] // bw, x0 + hit[0] % bw] = 1.0
            added += 1
            if np.flatnonzero(free.ravel())[0] != hit[0]:
                passed_a_hole += 1
    return out, added, passed_a_hole


def cloud(mp, depth, bgr, dx0, dy0, cam):
    """get_points_from_pixels + get_features with the raw colour features (ref src/pcd_generator.cpp:297-321, 336-380):
    the pixels of the map that have a depth, in scan order -> (positions n x 3, features n x 5), float32.
    cam: depth scale, fx, fy, cx, cy."""
    scale, fx, fy, cx, cy = (f32(v) for v in cam)
    ys, xs = np.nonzero((np.asarray(mp) != 0) & (np.asarray(depth) != 0))
    z = depth[ys, xs].astype(f32) / scale
    pos = np.stack([(xs.astype(f32) - cx) * z / fx, (ys.astype(f32) - cy) * z / fy, z], axis=1).astype(f32)
    feat = np.concatenate([bgr[ys, xs].astype(f32), dx0[ys, xs][:, None], dy0[ys, xs][:, None]], axis=1).astype(f32)
    return pos.reshape(-1, 3), feat.reshape(-1, 5)
