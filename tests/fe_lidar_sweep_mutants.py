"""Mutants of the restatement of the sweep contract (tests/fe_lidar_sweep_ref.py): each one restates the phase and the
move with one plausible device error in it -- the sign of the interval, the halves of the twist exchanged, the
translation without its rotation terms, a series cut short, a clamp, a floor or a fix-up of the azimuth left out, the
time word read as the other type or from the wrong place, and the twist of the frame before.
tests/test_fe_lidar_sweep_cpu.py holds that the scans made on purpose tell every one of them from the restatement: a
kernel with that error would fail the comparisons of tests/test_gpu_fe_lidar_sweep.py.  Python only; nothing here ever
runs against the GPU."""
import numpy as np

import fe_lidar_ref as K
import fe_lidar_sweep_ref as S

f32 = np.float32


def _phase(rec, sw, no_clamp=False, u32_as_float=False, float_as_u32=False, origin_after=False, no_direction=False,
           no_swap=False, no_x=False, no_y=False, tie_other=False, no_floor=False, offset_12=False):
    x, y, z = rec[:, 0], rec[:, 1], rec[:, 2]
    alive = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    clamp = (lambda s: s) if no_clamp else (lambda s: np.minimum(np.maximum(s, f32(0)), f32(1)))
    with np.errstate(all="ignore"):
        if sw.mode in (S.TIME_F32, S.TIME_U32):
            words = S.time_words(rec, sw._replace(time_offset=12) if offset_12 else sw)
            as_float = (sw.mode == S.TIME_F32) != (u32_as_float or float_as_u32)
            if as_float:
                t = words.view(f32)
                alive &= np.isfinite(t)
            else:
                t = words.astype(f32)
            if sw.mode == S.TIME_F32:
                s = t * f32(sw.time_scale) - f32(sw.time_origin) if origin_after else (t - f32(sw.time_origin)) * f32(sw.time_scale)
            else:
                s = t * f32(sw.time_scale)
            s = clamp(s)
        else:
            ax, ay = np.abs(x), np.abs(y)
            lo, hi = np.minimum(ax, ay), np.maximum(ax, ay)
            r = np.where(hi > 0, lo / hi, f32(0)).astype(f32)
            q = S.horner(S.ATAN, r * r) * r
            if not no_swap:
                q = np.where((ay >= ax) if tie_other else (ay > ax), f32(0.25) - q, q)
            if not no_x:
                q = np.where(x < 0, f32(0.5) - q, q)
            if not no_y:
                q = np.where(y < 0, -q, q)
            s = (f32(1) if no_direction else f32(sw.direction)) * q + f32(sw.phase0)
            if not no_floor:
                s = s - np.floor(s)
    return s.astype(f32), alive


def _move(p, s, s_ref, twist, reversed_a=False, swapped=False, tau_alone=False, no_c=False, short=False):
    tw = np.asarray(twist, f32)
    if swapped:
        tw = np.concatenate([tw[3:], tw[:3]])
    A_, B_, C_ = (S.SER_A[:-1], S.SER_B[:-1], S.SER_C[:-1]) if short else (S.SER_A, S.SER_B, S.SER_C)
    with np.errstate(all="ignore"):
        a = (f32(s_ref) - s) if reversed_a else (s - f32(s_ref))
        w = [a * tw[k] for k in range(3)]
        tau = [a * tw[3 + k] for k in range(3)]
        t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        A, B, C = S.horner(A_, t2), S.horner(B_, t2), S.horner(C_, t2)
        pk = [p[:, 0], p[:, 1], p[:, 2]]
        c1 = S.cross(w, pk)
        c2 = S.cross(w, c1)
        d1 = S.cross(w, tau)
        d2 = S.cross(w, d1)
        if tau_alone:
            out = [((pk[k] + A * c1[k]) + B * c2[k]) + tau[k] for k in range(3)]
        elif no_c:
            out = [((pk[k] + A * c1[k]) + B * c2[k]) + (tau[k] + B * d1[k]) for k in range(3)]
        else:
            out = [((pk[k] + A * c1[k]) + B * c2[k]) + ((tau[k] + B * d1[k]) + C * d2[k]) for k in range(3)]
    return np.stack(out, axis=1).astype(f32)


def _mutant(phase_kw=None, move_kw=None):
    def run(records, setting, cam, w, h, sw, twist):
        rec = np.asarray(records, f32)
        rec = rec if rec.ndim == 2 else np.zeros((0, 4), f32)
        s, alive = _phase(rec, sw, **(phase_kw or {}))
        moved = _move(rec[:, :3], s, sw.s_ref, twist, **(move_kw or {}))
        s = np.where(alive, s, f32(np.nan))
        moved = np.where(alive[:, None], moved, f32(np.nan))
        return K.lidar(moved, setting, cam, w, h) + (s, moved)
    return run


unchanged = _mutant()                                       # (no error: must equal the restatement, bit for bit)

FIELD, F32_ONLY, U32_ONLY, AZ, ALL = (S.TIME_F32, S.TIME_U32), (S.TIME_F32,), (S.TIME_U32,), (S.AZIMUTH,), (1, 2, 3)
# name -> (the mutant, the modes under which its error can show)
PLAIN = {
    "reversed_interval": (_mutant(None, dict(reversed_a=True)), ALL),      # s_ref - s for s - s_ref
    "twist_halves_swapped": (_mutant(None, dict(swapped=True)), ALL),      # w and v exchanged
    "translation_alone": (_mutant(None, dict(tau_alone=True)), ALL),       # tau without the B and C terms
    "no_C_term": (_mutant(None, dict(no_c=True)), ALL),
    "no_clamp": (_mutant(dict(no_clamp=True)), FIELD),
    "uint32_read_as_float": (_mutant(dict(u32_as_float=True)), U32_ONLY),
    "float_read_as_uint32": (_mutant(dict(float_as_u32=True)), F32_ONLY),
    "origin_after_scale": (_mutant(dict(origin_after=True)), F32_ONLY),
    "direction_ignored": (_mutant(dict(no_direction=True)), AZ),           # (shows under direction -1)
    "no_octant_swap": (_mutant(dict(no_swap=True)), AZ),
    "no_x_fixup": (_mutant(dict(no_x=True)), AZ),
    "no_y_fixup": (_mutant(dict(no_y=True)), AZ),
    "tie_the_other_way": (_mutant(dict(tie_other=True)), AZ),
    "no_floor": (_mutant(dict(no_floor=True)), AZ),
    "time_word_at_12": (_mutant(dict(offset_12=True)), FIELD),             # (shows where time_offset is not 12)
}
series_short = _mutant(None, dict(short=True))                            # every series one term short


def stale_twists(frames):
    """the frames of one context whose kernel moves by the twist of the frame BEFORE (the first frame: zero): one result
    of lidar_sweep per frame; `frames` holds lidar_sweep's arguments"""
    out, before = [], np.zeros(6, f32)
    for (records, setting, cam, w, h, sw, twist) in frames:
        out.append(S.lidar_sweep(records, setting, cam, w, h, sw, before))
        before = twist
    return out
