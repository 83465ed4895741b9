"""A plain restatement of the reference's pixel selector (ref thirdparty/PixelSelector2.cpp: computeHistQuantil,
makeHists, select, makeMaps; direction distribution off, thFactor 1, one recursion, a fresh selector at potential 3),
written from the reference's lines as loops over pixels.  It reads nothing of oracle/ and nothing of the product.

Arithmetic: every product, quotient and root the reference forms in float is formed here on np.float32 scalars.  The
three thresholds of a pixel depend on its 32x32 cell only and are formed once per cell; the planes' values are
compared as Python floats, which hold a float32 exactly (a comparison rounds nothing).

The one place the reference leaves undefined: a pixel with (xf>>5) == w/32 or (yf>>5) == h/32 reads thsSmoothed past
the (w/32)*(h/32) cells makeHists wrote.  Here every cell index past the end reads the LAST cell (the product's and
the oracle's choice, and what oracle/ref_selector_harness.cpp writes into the reference's slack with define_unwritten).

`mutant=`: one deliberate misreading each (MUTANTS); tests/test_selector_ref_cpu.py shows that the cases of
tests/selector_ref_cases.py tell every one of them from the reference.
"""
import numpy as np

f32 = np.float32

MUTANTS = (
    "ge_level0",            # >= in the level-0 running maximum: the last largest wins
    "ge_level1",            # ... level 1
    "ge_level2",            # ... level 2
    "columns_first",        # a B2's pixels visited column by column
    "b2_before_b3",         # B2 positions in the outer loop, B3 positions in the inner one
    "yf_ge",                # yf >= h-4 for yf > h-4
    "xf_ge4",               # xf >= w-4 for xf >= w-5
    "th2_unsquared",        # th2 = th1*dw1
    "level1_no_b4_mark",    # a level-1 hit no longer marks the B4
    "level0_marks_after",   # a level-0 hit marks its B3 only for the pixels after it
    "level1_index_floor",   # (int)(xf*0.5f) without the +0.25f   (equivalent: see OUT_OF_REACH)
    "median_add_after",     # + 7 after the smoothing
    "mean_double",          # sum/num and its square in double
    "quotia_wrong_pass",    # the sub-sampling quotient from the first pass's numHave
    "ideal_nearest",        # idealPotential rounded to nearest
    "charth_round",         # charTH rounded
    "pattern_ge",           # pattern[rn] >= charTH drops
    "rn_kept_only",         # rn advanced only for kept pixels
    "clamp_zero",           # cells past the end read 0 instead of the last cell
)

# mutants no input can tell from the reference, and why
OUT_OF_REACH = {
    "level1_index_floor": "for an integer xf >= 0, xf*0.5f is k or k+0.5 exactly, so (int)(xf*0.5f + 0.25f) == "
                          "(int)(xf*0.5f) == k: the +0.25f (and the +0.125 of level 2) changes no index",
}


def hist_quantile(hist, below):
    """computeHistQuantil (ref :59-68); bins past the 50 the caller clears are empty"""
    th = int(f32(hist[0]) * f32(below) + f32(0.5))
    for i in range(90):
        th -= hist[i + 1] if i + 1 < 50 else 0
        if th < 0:
            return i
    return 90


def make_hists(ag0, mutant=None):
    """makeHists (ref :71-136) -> (ths, thsSmoothed), (h/32, w/32) float32 each"""
    h, w = ag0.shape
    w32, h32 = w // 32, h // 32
    ths = np.zeros((h32, w32), f32)
    for y in range(h32):
        for x in range(w32):
            hist = [0] * 50
            for j in range(32):
                for i in range(32):
                    it, jt = i + 32 * x, j + 32 * y
                    if it > w - 2 or jt > h - 2 or it < 1 or jt < 1:
                        continue
                    g = int(np.sqrt(ag0[jt, it]))
                    if g > 48:
                        g = 48
                    hist[g + 1] += 1
                    hist[0] += 1
            q = hist_quantile(hist, 0.5)
            ths[y, x] = f32(q) if mutant == "median_add_after" else f32(q + 7)
    sm = np.zeros((h32, w32), f32)
    for y in range(h32):
        for x in range(w32):
            s, num = f32(0), f32(0)
            if x > 0:
                if y > 0:
                    num += f32(1); s += ths[y - 1, x - 1]
                if y < h32 - 1:
                    num += f32(1); s += ths[y + 1, x - 1]
                num += f32(1); s += ths[y, x - 1]
            if x < w32 - 1:
                if y > 0:
                    num += f32(1); s += ths[y - 1, x + 1]
                if y < h32 - 1:
                    num += f32(1); s += ths[y + 1, x + 1]
                num += f32(1); s += ths[y, x + 1]
            if y > 0:
                num += f32(1); s += ths[y - 1, x]
            if y < h32 - 1:
                num += f32(1); s += ths[y + 1, x]
            num += f32(1); s += ths[y, x]
            if mutant == "mean_double":
                m = np.float64(s) / np.float64(num)
                sm[y, x] = f32(m * m)
            elif mutant == "median_add_after":
                m = s / num + f32(7)
                sm[y, x] = m * m
            else:
                sm[y, x] = (s / num) * (s / num)
    return ths, sm


def select(ag0, ag1, ag2, ths_smoothed, pot, mutant=None):
    """select (ref :290-433) with thFactor 1 -> (map as a (h, w) float32 array, [n2, n3, n4])"""
    h, w = ag0.shape
    w1, w2, w32 = w // 2, w // 4, w // 32
    ncell = (w // 32) * (h // 32)
    dw1 = f32(0.75)
    dw2 = dw1 * dw1
    th_factor = f32(1)
    # the three thresholds of a cell, formed as the reference forms them per pixel
    cells = []
    for t in ths_smoothed.ravel():
        th0 = f32(t)
        th1 = th0 * dw1
        th2 = th1 * (dw1 if mutant == "th2_unsquared" else dw2)
        cells.append((float(th0 * th_factor), float(th1 * th_factor), float(th2 * th_factor)))
    past_end = (0.0, 0.0, 0.0) if mutant == "clamp_zero" else cells[ncell - 1]
    a0s, a1s, a2s = ag0.ravel().tolist(), ag1.ravel().tolist(), ag2.ravel().tolist()
    out = [0.0] * (w * h)
    ge0, ge1, ge2 = mutant == "ge_level0", mutant == "ge_level1", mutant == "ge_level2"
    y_edge = h - 5 if mutant == "yf_ge" else h - 4          # skipped when yf > y_edge
    x_edge = w - 4 if mutant == "xf_ge4" else w - 5         # skipped when xf >= x_edge
    quarter = f32(0.0) if mutant == "level1_index_floor" else f32(0.25)
    half, fourth, eighth = f32(0.5), f32(0.25), f32(0.125)
    i1x = [int(f32(x) * half + quarter) for x in range(w)]
    i1y = [int(f32(y) * half + quarter) for y in range(h)]
    i2x = [int(f32(x) * fourth + eighth) for x in range(w)]
    i2y = [int(f32(y) * fourth + eighth) for y in range(h)]
    big = float(f32(1e10))
    n2 = n3 = n4 = 0
    for y4 in range(0, h, 4 * pot):
        for x4 in range(0, w, 4 * pot):
            my3, mx3 = min(4 * pot, h - y4), min(4 * pot, w - x4)
            best_idx4, best_val4 = -1, 0.0
            # the B3s in the reference's order, each with its B2s -- or, for one mutant, the B2 position outside
            b3s = [(y3, x3) for y3 in range(0, my3, 2 * pot) for x3 in range(0, mx3, 2 * pot)]
            state3 = {b: [-1, 0.0, False] for b in b3s}     # bestIdx3, bestVal3, skip (one mutant only)
            if mutant == "b2_before_b3":
                visits = [(b, y2, x2) for y2 in (0, pot) for x2 in (0, pot) for b in b3s]
            else:
                visits = [(b, y2, x2) for b in b3s for y2 in (0, pot) for x2 in (0, pot)]
            last_b3 = None
            for b3, y2, x2 in visits:
                y3, x3 = b3
                x34, y34 = x3 + x4, y3 + y4
                my2, mx2 = min(2 * pot, h - y34), min(2 * pot, w - x34)
                if y2 >= my2 or x2 >= mx2:
                    continue
                if mutant != "b2_before_b3" and last_b3 is not None and last_b3 != b3:
                    # the B3 before this one is complete (ref :416-421)
                    st = state3[last_b3]
                    if st[0] > 0:
                        out[st[0]] = 2.0
                        best_val4 = big
                        n3 += 1
                    st[0] = -3   # (written)
                last_b3 = b3
                st = state3[b3]
                x234, y234 = x2 + x34, y2 + y34
                my1, mx1 = min(pot, h - y234), min(pot, w - x234)
                best_idx2, best_val2 = -1, 0.0
                if mutant == "columns_first":
                    pixels = [(y1, x1) for x1 in range(mx1) for y1 in range(my1)]
                else:
                    pixels = [(y1, x1) for y1 in range(my1) for x1 in range(mx1)]
                for y1, x1 in pixels:
                    xf, yf = x1 + x234, y1 + y234
                    idx = xf + w * yf
                    if xf < 4 or xf >= x_edge or yf < 4 or yf > y_edge:
                        continue
                    cell = (xf >> 5) + (yf >> 5) * w32
                    th0, th1, th2 = cells[cell] if cell < ncell else past_end
                    a0 = a0s[idx]
                    if a0 > th0:
                        if a0 > best_val2 or (ge0 and a0 >= best_val2):
                            best_val2, best_idx2 = a0, idx
                            if mutant == "level0_marks_after":
                                st[2] = True
                            else:
                                st[0] = -2
                            best_idx4 = -2
                    if st[0] == -2 or st[2]:
                        continue
                    a1 = a1s[i1x[xf] + i1y[yf] * w1]
                    if a1 > th1:
                        if a1 > st[1] or (ge1 and a1 >= st[1]):
                            st[1], st[0] = a1, idx
                            if mutant != "level1_no_b4_mark":
                                best_idx4 = -2
                    if best_idx4 == -2:
                        continue
                    a2 = a2s[i2x[xf] + i2y[yf] * w2]
                    if a2 > th2:
                        if a2 > best_val4 or (ge2 and a2 >= best_val4):
                            best_val4, best_idx4 = a2, idx
                if best_idx2 > 0:
                    out[best_idx2] = 1.0
                    st[1] = big
                    n2 += 1
            for b in b3s:   # the last B3 (every B3, for the mutant that interleaves them)
                st = state3[b]
                if st[0] > 0:
                    out[st[0]] = 2.0
                    best_val4 = big
                    n3 += 1
            if best_idx4 > 0:
                out[best_idx4] = 4.0
                n4 += 1
    return np.array(out, f32).reshape(h, w), [n2, n3, n4]


def make_maps(ag0, ag1, ag2, num_want, pattern, mutant=None, memo=None):
    """makeHists + makeMaps (ref :137-286) on a fresh selector -> dict(map, count, pot_used, reselected, ths,
    ths_smoothed, num_have, char_th): num_have is the final pass's count before the sub-sampling, char_th its
    threshold (None when it does not run).  `memo`: a dict the caller keeps for ONE set of planes and one mutant; the
    thresholds and the selection passes (which do not depend on num_want) are then computed once per potential."""
    ag0, ag1, ag2 = (np.ascontiguousarray(a, f32) for a in (ag0, ag1, ag2))
    h, w = ag0.shape
    memo = {} if memo is None else memo
    if "hists" not in memo:
        memo["hists"] = make_hists(ag0, mutant)
    ths, sm = memo["hists"]
    num_want = f32(num_want)
    pot, recursions, first_have = 3, 1, None
    with np.errstate(divide="ignore", invalid="ignore"):
        while True:
            if pot not in memo:
                memo[pot] = select(ag0, ag1, ag2, sm, pot, mutant)
            mp, n = memo[pot][0].copy(), memo[pot][1]
            num_have = f32(n[0] + n[1] + n[2])
            if first_have is None:
                first_have = num_have
            quotia = num_want / num_have
            K = num_have * f32(pot + 1) * f32(pot + 1)
            root = np.sqrt(K / num_want) - f32(1)
            ideal = int(np.rint(root)) if mutant == "ideal_nearest" else int(root)
            if ideal < 1:
                ideal = 1
            if recursions > 0 and float(quotia) > 1.25 and pot > 1:
                if ideal >= pot:
                    ideal = pot - 1
                pot, recursions = ideal, recursions - 1
                continue
            if recursions > 0 and float(quotia) < 0.25:
                if ideal <= pot:
                    ideal = pot + 1
                pot, recursions = ideal, recursions - 1
                continue
            break
        if mutant == "quotia_wrong_pass":
            quotia = num_want / first_have
    count, char_th = int(num_have), None
    if float(quotia) < 0.95:
        v = f32(255) * quotia
        char_th = (int(np.rint(v)) if mutant == "charth_round" else int(v)) & 0xFF
        flat = mp.ravel()
        rn = 0
        for i in range(w * h):
            if flat[i] != 0:
                drop = pattern[rn] >= char_th if mutant == "pattern_ge" else pattern[rn] > char_th
                if drop:
                    flat[i] = 0
                    count -= 1
                if mutant != "rn_kept_only" or not drop:
                    rn += 1
    return {"map": mp, "count": count, "pot_used": pot, "reselected": 1 - recursions, "ths": ths, "ths_smoothed": sm,
            "num_have": int(num_have), "char_th": char_th}
