"""Mutants of the restatement of the infill contract (tests/fe_infill_ref.py): each one restates the stage with one
plausible device error in it -- the errors a tiled, two-pass interpolation of inverse depth can make: the wrong mean, the
wrong rounding, the weights the wrong way round, a product that wraps, the limit on the run's length read as a limit on
something else, the border or a refused end taken for an end, the passes in the wrong order or on the wrong plane, a
sweep in place, ends lost where two tiles meet.
tests/test_fe_infill_cpu.py holds that the planes made on purpose tell every one of them from the restatement, and names
the plane and the settings: a kernel with that error would fail the byte comparison of tests/test_gpu_fe_infill.py.
Python only; nothing here ever runs against the GPU."""
import numpy as np

import fe_infill_ref as K


def one_pass(X, g, jump_rel, value=K.value, candidate=None, border=False, strict=True, rel_hi=False, in_place=False):
    """K.pass_loop with its rules open to change, pixel by pixel: `candidate(da, db, g)` in place of da + db - 1 <= g;
    `border`: a run that touches the border is bounded by its one end, twice; `strict` False: >= in the jump test;
    `rel_hi`: the step relative to hi; `in_place`: a pixel filled is an end to the pixels behind it"""
    X = np.asarray(X)
    h, w = X.shape
    src = [[int(v) for v in row] for row in X]
    out = [row[:] for row in src]
    ref = np.zeros((h, w), bool)
    candidate = candidate or (lambda da, db, g: da + db - 1 <= g)
    j = np.float32(jump_rel)
    for y in range(h):
        line = out[y] if in_place else src[y]
        for x in range(w):
            if src[y][x] != 0 or g == 0:
                continue
            ia = next((i for i in range(x - 1, -1, -1) if line[i] != 0), None)
            ib = next((i for i in range(x + 1, w) if line[i] != 0), None)
            if border and (ia is None) != (ib is None):
                end = line[ia if ib is None else ib]
                A, B = end, end
                da, db = (x + 1, ib - x) if ia is None else (x - ia, w - x)
            elif ia is None or ib is None:
                continue
            else:
                A, B, da, db = line[ia], line[ib], x - ia, ib - x
            if not candidate(da, db, g):
                continue
            lo, hi = min(A, B), max(A, B)
            step, edge = np.float32(hi - lo), j * np.float32(hi if rel_hi else lo)
            if j > 0 and (step > edge if strict else step >= edge):
                ref[y, x] = True
                continue
            out[y][x] = int(value(A, B, da, db)) & 0xFFFF
    return np.array(out, np.int64).reshape(h, w), ref


def _two(S, f, rows=None, cols=None):
    """the stage from two passes with rules of their own (keyword arguments of one_pass)"""
    S = np.asarray(S)
    H, rr = one_pass(S, f[0], f[2], **(rows or {}))
    Ft, rc = one_pass(H.T, f[1], f[2], **(cols if cols is not None else rows or {}))
    return K.finish(S, H, Ft.T, rr, rc.T)


def linear(S, f):
    """linear in depth, rounded half up"""
    return _two(S, f, dict(value=lambda A, B, da, db: (2 * (A * db + B * da) + (da + db)) // (2 * (da + db))))


def floor(S, f):
    """floor(N / Dn): no rounding"""
    return _two(S, f, dict(value=lambda A, B, da, db: (A * B * (da + db)) // (A * da + B * db)))


def weights_swapped(S, f):
    """Dn = A db + B da"""
    return _two(S, f, dict(value=lambda A, B, da, db: K.value(A, B, db, da)))


def product_32(S, f):
    """N in 32 bits"""
    def value(A, B, da, db):
        N, Dn = (A * B * (da + db)) & 0xFFFFFFFF, A * da + B * db
        return (2 * N + Dn) // (2 * Dn)
    return _two(S, f, dict(value=value))


def sum_for_length(S, f):
    """L <= g read as da + db <= g"""
    return _two(S, f, dict(candidate=lambda da, db, g: da + db <= g))


def per_side(S, f):
    """L <= g read as da <= g and db <= g, without the sum"""
    return _two(S, f, dict(candidate=lambda da, db, g: da <= g and db <= g))


def border_end(S, f):
    """the border as an end: a run that touches it is bridged from its one end"""
    return _two(S, f, dict(border=True))


def not_strict(S, f):
    """>= for > in the jump test"""
    return _two(S, f, dict(strict=False))


def relative_to_hi(S, f):
    """the step taken relative to hi"""
    return _two(S, f, dict(rel_hi=True))


def columns_on_s(S, f):
    """the column pass reads S: F is H where H has a depth, else what the column pass makes of S"""
    S = np.asarray(S)
    H, rr = K.pass_np(S, f[0], f[2])
    Ct, rc = K.pass_np(S.T, f[1], f[2])
    return K.finish(S, H, np.where(H != 0, H, Ct.T), rr, rc.T)


def columns_first(S, f):
    """the column pass first, the row pass on its output; the flags by the pass that filled"""
    S = np.asarray(S)
    Ct, rc = K.pass_np(S.T, f[1], f[2])
    C = Ct.T
    F, rr = K.pass_np(C, f[0], f[2])
    flags = np.where((S == 0) & (C != 0), K.COL, 0) + np.where((C == 0) & (F != 0), K.ROW, 0) + \
        np.where((F == 0) & (rr | rc.T), K.JUMP, 0)
    return F.astype(np.uint16), flags.astype(np.uint8), int(np.count_nonzero(flags == K.ROW)), int(np.count_nonzero(flags == K.COL))


def in_place(S, f):
    """each pass swept in place"""
    return _two(S, f, dict(in_place=True))


def limits_swapped(S, f):
    """gap_y along the rows, gap_x down the columns"""
    return K.infill(S, (f[1], f[0], f[2]))


def tile_cut(S, f, tw, th):
    """every tile of tw x th pixels on its own: an end outside the pixel's tile is lost, no halo"""
    S = np.asarray(S)
    h, w = S.shape
    F, flags = np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint8)
    for y0 in range(0, h, th):
        for x0 in range(0, w, tw):
            F[y0:y0 + th, x0:x0 + tw], flags[y0:y0 + th, x0:x0 + tw] = K.infill(S[y0:y0 + th, x0:x0 + tw], f)[:2]
    return F, flags, int(np.count_nonzero(flags == K.ROW)), int(np.count_nonzero(flags == K.COL))


TILES = [K.TILE, (32, 8), (16, 16), (64, 4)]
