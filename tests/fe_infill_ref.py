"""A restatement of the front end's infill contract (include/cvo_frontend.h, at cvo_fe_depth_infill): integer planes,
and one float32 product in the jump test.  infill_loop() is the contract read out run by run in Python integers,
infill() the vectorised form; the CPU test holds the one to the other.  k_fe_infill of csrc/cvo_infill.hip is held to
infill() by bytes.

Settings here are (gap_x, gap_y, jump_rel) triples, or None: no stage.
Also here: the planes made on purpose, the settings and the frames the tests share."""
import numpy as np

ROW, COL, JUMP = 1, 2, 4
TILE = (64, 16)     # k_fe_infill's tile, width x height
GAPS = [(0, 0), (1, 0), (0, 1), (2, 5), (15, 0), (0, 31), (15, 31)]
JUMPS = [0.0, 0.25]
SETTINGS = [(gx, gy, j) for gx, gy in GAPS for j in JUMPS]
SIZES = [(96, 64), (127, 193)]          # width x height: no multiple of the tile, more than one tile each way
LENGTHS = [1, 2, 3, 5, 6, 15, 16, 31, 32]   # g and g + 1 for every g of GAPS
FRAME_SETTINGS = [(2, 5, 0.25), (15, 31, 0.0), (1, 0, 0.0), (0, 1, 0.25)]
# the ground plane of the issue: a camera 1.65 m above it, fy 721, cy 180, 256 units per metre
GROUND_FY, GROUND_CY, GROUND_HEIGHT, GROUND_SCALE = 721.0, 180.0, 1.65, 256.0
GROUND_ROWS = (200, 369)                # the image rows the ground plane is made on
POLES = ((30, 33, 1280), (70, 72, 2048))    # columns [x0, x1) at a depth, in front of the ground


def to_struct(F, f):
    """The settings as the package's DepthInfill."""
    return None if f is None else F.DepthInfill(*f)


def bad_infills():
    """settings cvo_fe_check_depth_infill refuses, as (gap_x, gap_y, jump_rel, pad_)"""
    return [(-1, 0, 0.0, 0), (16, 0, 0.0, 0), (0, -1, 0.0, 0), (0, 32, 0.0, 0), (2, 5, -0.5, 0), (2, 5, float("nan"), 0),
            (2, 5, float("inf"), 0), (2, 5, 0.25, 1)]


def value(A, B, da, db):
    """floor((2 N + Dn) / (2 Dn)): works on Python integers and on int64 arrays alike"""
    N = A * B * (da + db)
    Dn = A * da + B * db
    return (2 * N + Dn) // (2 * Dn)


def refused(lo, hi, jump_rel):
    """the jump test: one float32 multiplication and one comparison"""
    j = np.float32(jump_rel)
    return bool(j > 0) & (np.asarray(hi - lo).astype(np.float32) > j * np.asarray(lo).astype(np.float32))


def pass_loop(X, g, jump_rel):
    """One pass along the rows of X (a list of rows of Python integers would do): (the output, the pixels of refused
    runs), run by run in the words of the contract"""
    X = np.asarray(X)
    h, w = X.shape
    out = [[int(v) for v in row] for row in X]
    ref = np.zeros((h, w), bool)
    for y in range(h):
        ends = [int(i) for i in np.flatnonzero(X[y])]
        for ia, ib in zip(ends[:-1], ends[1:]):         # (a run in front of the first or behind the last is not bounded)
            L = ib - ia - 1
            if L < 1 or L > g:
                continue
            A, B = out[y][ia], out[y][ib]
            if refused(min(A, B), max(A, B), jump_rel):
                ref[y, ia + 1:ib] = True
                continue
            for x in range(ia + 1, ib):
                out[y][x] = value(A, B, x - ia, ib - x)
    return np.array(out, np.int64).reshape(h, w), ref


def pass_np(X, g, jump_rel):
    """The same, vectorised"""
    X = np.asarray(X).astype(np.int64)
    h, w = X.shape
    idx = np.broadcast_to(np.arange(w), (h, w))
    have = X != 0
    ia = np.maximum.accumulate(np.where(have, idx, -1), axis=1)
    ib = np.minimum.accumulate(np.where(have, idx, w)[:, ::-1], axis=1)[:, ::-1]
    bounded = ~have & (ia >= 0) & (ib < w)
    A = np.take_along_axis(X, np.clip(ia, 0, w - 1), axis=1)
    B = np.take_along_axis(X, np.clip(ib, 0, w - 1), axis=1)
    da, db = idx - ia, ib - idx
    cand = bounded & (da + db - 1 <= g)
    A, B, da, db = (np.where(cand, a, 1) for a in (A, B, da, db))
    ref = cand & refused(np.minimum(A, B), np.maximum(A, B), jump_rel)
    return np.where(cand & ~ref, value(A, B, da, db), X), ref


def finish(S, H, F, ref_row, ref_col):
    """(F uint16, INFILL uint8, the number of ROW pixels, the number of COL pixels) of the contract"""
    S = np.asarray(S)
    F = np.asarray(F)
    assert F.min() >= 0 and F.max() <= 65535
    row = (S == 0) & (H != 0)
    col = (H == 0) & (F != 0)
    jump = (F == 0) & (ref_row | ref_col)
    flags = (np.where(row, ROW, 0) + np.where(col, COL, 0) + np.where(jump, JUMP, 0)).astype(np.uint8)
    return F.astype(np.uint16), flags, int(np.count_nonzero(row)), int(np.count_nonzero(col))


def _infill(S, f, one_pass):
    S = np.asarray(S)
    assert S.dtype == np.uint16 and S.ndim == 2
    gx, gy, jump_rel = f
    H, ref_row = one_pass(S, gx, jump_rel)
    Ft, ref_col = one_pass(H.T, gy, jump_rel)           # (the column pass reads H)
    return finish(S, H, Ft.T, ref_row, ref_col.T)


def infill(S, f):
    """The contract on a whole plane: (F, INFILL, row_filled, col_filled)"""
    return _infill(S, f, pass_np)


def infill_loop(S, f):
    """The same from the loop over runs (slow: small planes only)"""
    return _infill(S, f, pass_loop)


# ---- the planes made on purpose ------------------------------------------------------------------------

def _surface(w, h):
    """a smooth surface without holes: neighbouring pixels differ by less than one per cent"""
    return (3000 + 7 * np.arange(w)[None, :] + 11 * np.arange(h)[:, None]).astype(np.uint16)


def _starts(L, seam, last):
    """where a run of L pixels begins: inside the first tile, and across the seam behind pixel seam - 1"""
    inside = min(2 + L % 7, seam - 1 - L) if L < seam - 2 else 1
    return max(inside, 1), min(max(seam - (L + 1) // 2, 1), last - L)


def row_runs(w, h):
    """runs of every length of LENGTHS in rows of their own, two rows apart: one inside tile column 0, one across the
    seam x = 63|64; on a surface, so that every run is bounded"""
    X = _surface(w, h)
    y = 1
    for L in LENGTHS:
        for x0 in _starts(L, TILE[0], w - 1):
            assert x0 >= 1 and x0 + L <= w - 1 and y < h - 1
            X[y, x0:x0 + L] = 0
            y += 2
    return X


def col_runs(w, h):
    """the same in columns of their own, three columns apart: one beginning in tile row 1 (a run longer than 14 pixels
    cannot lie inside a tile), one across the seam y = 15|16; in a plane higher than 64 rows a second set 64 rows
    from the lower border, across the last seams"""
    X = _surface(w, h)
    x = 1
    for L in LENGTHS:
        for y0 in (min(TILE[1] + 1, h - 2 - L), _starts(L, TILE[1], h - 1)[1]):
            assert y0 >= 1 and y0 + L <= h - 1 and x < w - 1
            X[y0:y0 + L, x] = 0
            if h > 64 + 2:
                X[h - 64 + y0:h - 64 + y0 + L, x] = 0
            x += 3
    return X


def borders(w, h):
    """runs of one and two pixels that touch each border (they stay holes) and runs one pixel away from it (bridged),
    on a surface"""
    X = _surface(w, h)
    for k, L in enumerate((1, 2)):
        y, x = 5 + 8 * k, 20 + 8 * k
        X[y, 0:L] = 0;             X[y + 2, 1:1 + L] = 0            # the left border
        X[y + 4, w - L:w] = 0;     X[y + 6, w - 1 - L:w - 1] = 0    # the right one
        X[0:L, x] = 0;             X[1:1 + L, x + 2] = 0            # the upper one
        X[h - L:h, x + 4] = 0;     X[h - 1 - L:h - 1, x + 6] = 0    # the lower one
    return X


def _lines(w, h, patterns):
    """every pattern once along a row and once along a column of a plane that is otherwise empty.  Row patterns in
    rows 1, 3, ..., the even ones inside tile column 0, the odd ones across the seam x = 63|64; column patterns below
    them from row 14 on, one under the other in columns of their own at the right border, the first across the seam
    y = 15|16.  No row holds two column patterns and no row pattern comes within 16 pixels of one."""
    X = np.zeros((h, w), np.uint16)
    assert 2 * len(patterns) < 14
    y0 = 14
    for k, p in enumerate(patterns):
        n = len(p)
        x0 = 3 + 18 * (k // 2) if k % 2 == 0 else TILE[0] - n // 2
        assert x0 + n + 16 < w - 2 * len(patterns) and (k % 2 == 1 or x0 + n < TILE[0])
        X[1 + 2 * k, x0:x0 + n] = p
        assert y0 + n < h
        X[y0:y0 + n, w - 2 - 2 * k] = p
        y0 += n + 1
    return X


JUMP_PATTERNS = [(4000, 0, 5000), (5000, 0, 4000), (4000, 0, 5001), (5001, 0, 4000)]
ARITHMETIC_PATTERNS = [(1, 0, 2), (1, 0, 3), (3, 0, 0, 6), (1, 0, 65535), (65535,) + (0,) * 15 + (65535,)]


def jumps(w, h):
    """4000|5000 and 4000|5001 over a hole of one pixel, both orders, in a row and in a column"""
    return _lines(w, h, JUMP_PATTERNS)


def arithmetic(w, h):
    """ends (1, 2), (1, 3), (3, 6) over two pixels, (1, 65535), and 65535 twice over fifteen pixels in a row and a
    column and over thirty-one in a column"""
    X = _lines(w, h, ARITHMETIC_PATTERNS)
    X[12:45, 60] = (65535,) + (0,) * 31 + (65535,)
    return X


def columns_read_h(w, h):
    """two lines: in the upper one a one-pixel gap the row pass closes; one column below that gap a hole of one pixel
    and a depth under it.  The column's upper end exists only in H.  Once inside a tile, once across both seams."""
    X = np.zeros((h, w), np.uint16)
    for x, y in ((20, 4), (TILE[0] - 1, TILE[1] - 1), (TILE[0] + 8, TILE[1] - 2)):
        X[y, x - 1], X[y, x + 1], X[y + 2, x] = 4000, 4400, 4100
    return X


def not_in_place(w, h):
    """4000, 0, 0, 5000 in a row and in a column: swept in place the second hole sees the first one's new value"""
    return _lines(w, h, [(4000, 0, 0, 5000), (5000, 0, 0, 4000)])


def ground_truth(w, h):
    """(the true rounded depth of the ground plane at every pixel of the plane, 0 where it is not made; the image row
    of every row of the plane).  The plane's last row is image row 369, or its first one image row 200 in a plane of
    fewer rows than lie between them; the ground is made on image rows 200 to 369."""
    rows = np.arange(h) + min(GROUND_ROWS[0], GROUND_ROWS[1] - (h - 1))
    made = (rows >= GROUND_ROWS[0]) & (rows <= GROUND_ROWS[1])
    z = np.where(made, np.rint(GROUND_FY * GROUND_HEIGHT * GROUND_SCALE / np.where(made, rows - GROUND_CY, 1.0)), 0)
    assert z.max() <= 65535
    return np.broadcast_to(z[:, None], (h, w)).astype(np.uint16), rows


def ground(w, h):
    """a scan of the ground plane: lines every 5 image rows with every fourth pixel missing, and two poles in front"""
    truth, rows = ground_truth(w, h)
    X = np.where((rows % 5 == 0)[:, None] & (np.arange(w) % 4 != 3)[None, :], truth, 0).astype(np.uint16)
    for x0, x1, z in POLES:
        X[:, x0:x1] = np.where((rows % 5 == 0) & (truth[:, 0] != 0), z, 0)[:, None]
    return X


def ground_pixels(w, h):
    """where a filled pixel of ground() lies on the ground alone: two columns clear of every pole"""
    keep = np.ones(w, bool)
    for x0, x1, _ in POLES:
        keep[max(x0 - 2, 0):x1 + 2] = False
    return np.broadcast_to(keep[None, :], (h, w))


def sparse(w, h, seed=5):
    """a scene of three surfaces with two thirds of its pixels dropped at random: runs of every short length in both
    directions in every tile, and steps for the jump test"""
    rng = np.random.default_rng(seed)
    X = _surface(w, h).astype(np.int64)
    X[:, w // 3:] += 2500
    X[h // 2:, :] = X[h // 2:, :] * 2
    X = np.where(rng.random((h, w)) < 0.34, X, 0)
    X[rng.integers(0, h, 12), rng.integers(0, w, 12)] = 65535
    X[rng.integers(0, h, 12), rng.integers(0, w, 12)] = 1
    return np.clip(X, 0, 65535).astype(np.uint16)


MAKERS = {"row-runs": row_runs, "col-runs": col_runs, "borders": borders, "jumps": jumps, "arithmetic": arithmetic,
          "columns-read-h": columns_read_h, "not-in-place": not_in_place, "ground": ground, "sparse": sparse}
MADE_NAMES = ["%s-%dx%d" % (name, w, h) for name in MAKERS for w, h in SIZES]
_MADE = {}


def plane(name):
    """the made plane of that name, e.g. "jumps-96x64"; made once and left unchanged"""
    if name not in _MADE:
        kind, size = name.rsplit("-", 1)
        w, h = (int(v) for v in size.split("x"))
        X = MAKERS[kind](w, h)
        assert X.dtype == np.uint16 and X.shape == (h, w)
        X.setflags(write=False)
        _MADE[name] = X
    return _MADE[name]


def made(name, f):
    """(S, F, INFILL, row_filled, col_filled) of a made plane at settings f; computed once"""
    key = (name, f)
    if key not in _MADE:
        out = (plane(name),) + infill(plane(name), f)
        for a in out[1:3]:
            a.setflags(write=False)
        _MADE[key] = out
    return _MADE[key]


def long_plane(w, h, seed=9):
    """a plane of 8192 x 3 or 3 x 8192: sparse along its long side, so that runs cross many seams"""
    return sparse(w, h, seed)


def spoil(depth, seed):
    """a dense depth image thinned as a scan thins it: every third row kept, and of those every fourth pixel dropped"""
    depth = np.asarray(depth)
    h, w = depth.shape
    keep = (np.arange(h) % 3 == seed % 3)[:, None] & (np.arange(w) % 4 != seed % 4)[None, :]
    return np.where(keep, depth, 0).astype(np.uint16)
