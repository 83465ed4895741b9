"""Wrong versions of the photometric stage (the photometric contract of include/cvo_frontend.h), each the restatement
tests/fe_photometric_ref.py with one mistake kernels of this shape -- four pixels per thread from whole dwords, a table
in LDS, integer sums per block, a single-thread tail -- could make.  Each is a set of steps for fe_photometric_ref.frame().
tests/test_fe_photometric_cpu.py shows for each an input of the GPU test that tells it from the restatement."""
import numpy as np

import fe_photometric_ref as P

U = np.uint64


def values_table_rgb(bgr, response, vignette):
    """the table indexed in R, G, B order"""
    return P.values(bgr, None if response is None else response[::-1], vignette)


def values_vignette_rows_by_height(bgr, response, vignette):
    """the vignette's row length taken from the height: pixel (x, y) reads entry y * h + x"""
    if vignette is None:
        return P.values(bgr, response, vignette)
    h, w = vignette.shape
    yy, xx = np.mgrid[0:h, 0:w]
    return P.values(bgr, response, vignette.reshape(-1)[np.minimum(yy * h + xx, w * h - 1)])


def correct_truncates(A, G):
    return np.minimum((A * np.array(G, U)) >> U(32), U(255)).astype(np.uint8)


def correct_wraps(A, G):
    """no clamp at 255"""
    return (((A * np.array(G, U) + U(1 << 31)) >> U(32)) & U(255)).astype(np.uint8)


def correct_rounds_between(A, G):
    """A rounded to Q8 between V and G"""
    a = (A + U(2048)) >> U(12)
    return np.minimum((a * np.array(G, U) + U(1 << 19)) >> U(20), U(255)).astype(np.uint8)


def correct_tail_skipped(bgr):
    """the last np % 4 pixels are left as they were"""
    def step(A, G):
        out = P.correct(A, G).reshape(-1, 3)
        n = len(out)
        if n % 4:
            out[n - n % 4:] = bgr.reshape(-1, 3)[n - n % 4:]
        return out.reshape(A.shape)
    return step


def stat_window_on_corrected(bgr, A, lo, hi):
    """the window tested on the linearised, vignette-corrected value"""
    v = np.minimum(A >> U(20), U(255)).astype(np.int64)
    inside = ((v >= lo) & (v <= hi)).all(axis=-1)
    return int(inside.sum()), tuple(int((A[..., c][inside] >> U(12)).sum(dtype=U)) for c in range(3))


def stat_counts_channels(bgr, A, lo, hi):
    """k counts the channels of the counted pixels"""
    k, M = P.stat(bgr, A, lo, hi)
    return 3 * k, M


def stat_lo_exclusive(bgr, A, lo, hi):
    inside = ((bgr > lo) & (bgr <= hi)).all(axis=-1)
    return int(inside.sum()), tuple(int((A[..., c][inside] >> U(12)).sum(dtype=U)) for c in range(3))


def stat_shift_20(bgr, A, lo, hi):
    inside = ((bgr >= lo) & (bgr <= hi)).all(axis=-1)
    return int(inside.sum()), tuple(int((A[..., c][inside] >> U(20)).sum(dtype=U)) for c in range(3))


def solve_common_from_channel_0(s, k, M, state, rearm=False):
    if s[4]:
        return P.solve(s, k, M, state, rearm)
    G, flags, T, new = P.solve(s, k, M, state, rearm)
    if flags == 0 and M[0]:
        held = tuple(s[5]) if any(s[5]) else state[1]
        G = (P.clamp((held[0] * k * 4096 + (M[0] >> 1)) // M[0], s),) * 3
    return G, flags, T, new


def solve_lock_reopened(s, k, M, state, rearm=False):
    """the lock re-opened every frame"""
    return P.solve(s, k, M, P.OPEN, rearm)


def solve_no_fallback(s, k, M, state, rearm=False):
    """no fallback under min_count"""
    return P.solve(s[:3] + (1 if k else s[3],) + s[4:], k, M, state, rearm)


def solve_no_gain_clamp(s, k, M, state, rearm=False):
    return P.solve(s[:6] + (1, 1 << 62) + s[8:], k, M, state, rearm)


# steps by name: what frame() takes in place of its own; callables of the image where the step needs it
STEPS = {
    "table_rgb": dict(values=values_table_rgb),
    "vignette_rows_by_height": dict(values=values_vignette_rows_by_height),
    "truncates": dict(correct=correct_truncates),
    "wraps": dict(correct=correct_wraps),
    "rounds_between": dict(correct=correct_rounds_between),
    "window_on_corrected": dict(stat=stat_window_on_corrected),
    "counts_channels": dict(stat=stat_counts_channels),
    "lo_exclusive": dict(stat=stat_lo_exclusive),
    "common_from_channel_0": dict(solve=solve_common_from_channel_0),
    "shift_20": dict(stat=stat_shift_20),
    "no_fallback": dict(solve=solve_no_fallback),
    "no_gain_clamp": dict(solve=solve_no_gain_clamp),
}
# ... told apart by the lock's sequence, by the pair, and by a size that is no multiple of four
SEQUENCE = {"lock_reopened": dict(solve=solve_lock_reopened)}


def pair_right_statistic(left, right, s, response, vignette):
    """the statistic taken from the right image"""
    return P.frame(left, s, response, vignette, None, right=right, stat_image=right)
