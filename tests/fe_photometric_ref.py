"""The photometric contract of include/cvo_frontend.h (at cvo_fe_photometric), restated in numpy and Python integers:
what k_fe_photo_apply, k_fe_photo_stat and k_fe_photo_gain of csrc/cvo_photo.hip must give by bytes and by value.  Also
the inputs the GPU test (tests/test_gpu_fe_photometric.py) runs them on: cases(), auto_sequence(), pair().

A setting is the tuple (flags, lo, hi, min_count, per_channel, target, gain_min, gain_max, pad_) of the structure; a
frame's record the dict of cvo_fe_photometric_frame; the state between frames of AUTO (locked, T).  frame() takes its four
steps as arguments, so that tests/fe_photometric_mutants.py can put a wrong one in the place of one of them."""
import numpy as np

RESPONSE, VIGNETTE, GAIN, AUTO = 1, 2, 4, 8
FALLBACK, LOCKED = 1, 2
UNITY = 4096
SIZES = ((1, 1), (2, 1), (3, 2), (5, 3), (13, 7), (66, 18), (130, 34), (64, 64), (8192, 1), (1, 8192))
OPEN = (False, (0, 0, 0))                       # the state a setter leaves: the lock open


def setting(flags, lo=8, hi=247, min_count=1, per_channel=0, target=(0, 0, 0), gain_min=256, gain_max=65535, pad=0):
    return (flags, lo, hi, min_count, per_channel, tuple(target), gain_min, gain_max, pad)


def to_struct(F, s):
    return F.Photometric(*s)


def check(s, have_response, have_vignette):
    """cvo_fe_check_photometric"""
    if s is None:
        return False
    flags, lo, hi, min_count, per_channel, target, gmin, gmax, pad = s
    if flags == 0 or flags > 15 or flags < 0 or pad != 0 or (flags & GAIN and flags & AUTO):
        return False
    if not 0 <= lo <= hi <= 255 or min_count < 1 or per_channel not in (0, 1):
        return False
    if any(t > 65535 for t in target) or not 1 <= gmin <= gmax <= 65535:
        return False
    return bool(have_response) == bool(flags & RESPONSE) and bool(have_vignette) == bool(flags & VIGNETTE)


def gain_q12(gain):
    """G of cvo_fe_set_photometric_gain, before the clamp: each operation in float32"""
    return int(np.uint32(np.float32(np.float32(gain) * np.float32(4096.0)) + np.float32(0.5)))


def gain_ok(gain):
    g = np.float32(gain)
    return bool(np.isfinite(g)) and np.float32(0.0625) <= g <= np.float32(15.99)


def response_table(inv):
    """cvo_fe_response_table, or None where it refuses"""
    v = np.asarray(inv, np.float32)
    if v.shape != (256,) or not np.isfinite(v).all() or (v < 0).any() or (v > 255).any():
        return None
    q = (v * np.float32(256.0) + np.float32(0.5)).astype(np.uint32)
    return np.minimum(q, 65535).astype(np.uint16)


def vignette_gains(atten):
    a = np.asarray(atten, np.uint16).astype(np.int64)
    g = np.where(a > 0, (4096 * 65535 + a // 2) // np.maximum(a, 1), 65535)
    return np.minimum(g, 65535).astype(np.uint16)


# ---- the four steps -------------------------------------------------------------------------------------

def values(bgr, response, vignette):
    """A = L * V per pixel and channel, uint64 h x w x 3"""
    b = bgr.astype(np.int64)
    if response is None:
        L = b << 8
    else:
        L = np.stack([response[c].astype(np.int64)[b[..., c]] for c in range(3)], axis=-1)
    V = np.full(bgr.shape[:2], UNITY, np.int64) if vignette is None else vignette.astype(np.int64)
    return (L * V[..., None]).astype(np.uint64)


def stat(bgr, A, lo, hi):
    """k and M_c over the pixels whose three INPUT bytes lie in [lo, hi]"""
    inside = ((bgr >= lo) & (bgr <= hi)).all(axis=-1)
    k = int(inside.sum())
    M = tuple(int((A[..., c][inside] >> np.uint64(12)).sum(dtype=np.uint64)) for c in range(3))
    return k, M


def clamp(q, s):
    return min(max(q, s[6]), s[7])


def solve(s, k, M, state, rearm=False):
    """(G, flags, T of the record, the state behind the frame) of an AUTO frame"""
    _, _, _, min_count, per_channel, target, _, _, _ = s
    use_lock = not any(target)
    locked, held = state
    if rearm:
        locked = False
    T = (held if locked else (0, 0, 0)) if use_lock else tuple(target)
    G, flags = (UNITY,) * 3, 0
    if k < min_count:
        flags = FALLBACK
    elif use_lock and not locked:
        T = tuple((M[c] + (k >> 1)) // k for c in range(3))
        locked, flags = True, LOCKED
    elif per_channel:
        if 0 in M:
            flags = FALLBACK
        else:
            G = tuple(clamp((T[c] * k * 4096 + (M[c] >> 1)) // M[c], s) for c in range(3))
    else:
        Ms, Ts = sum(M), sum(T)
        if Ms == 0:
            flags = FALLBACK
        else:
            G = (clamp((Ts * k * 4096 + (Ms >> 1)) // Ms, s),) * 3
    new_state = (locked, T if use_lock and locked else (0, 0, 0))
    rec_T = (0, 0, 0) if use_lock and not locked else T
    return G, flags, rec_T, new_state


def correct(A, G):
    g = np.array(G, np.uint64)
    return np.minimum((A * g + np.uint64(1 << 31)) >> np.uint64(32), np.uint64(255)).astype(np.uint8)


def header_gains(s, gains_q12):
    """the header's gains: the caller's clamped under GAIN, else 4096"""
    if not s[0] & GAIN or gains_q12 is None:
        return (UNITY,) * 3
    return tuple(clamp(int(g), s) for g in gains_q12)


def frame(bgr, s, response=None, vignette=None, gains_q12=None, state=OPEN, rearm=False, right=None, stat_image=None,
          values=values, stat=stat, solve=solve, correct=correct):
    """One frame: (the corrected image, its record, the state behind it), and with `right` the corrected right image as
    a fourth.  `stat_image`: the image the statistic is taken from (the left one)."""
    A = values(bgr, response, vignette)
    if s[0] & AUTO:
        src = bgr if stat_image is None else stat_image
        k, M = stat(src, A if stat_image is None else values(src, response, vignette), s[1], s[2])
        G, flags, T, state = solve(s, k, M, state, rearm)
    else:
        G, flags, T, k, M = header_gains(s, gains_q12), 0, (0, 0, 0), 0, (0, 0, 0)
    rec = dict(gain=tuple(G), flags=flags, count=k, sum=tuple(M), target=tuple(T))
    out = correct(A, G)
    if right is None:
        return out, rec, state
    return out, rec, state, correct(values(right, response, vignette), G)


def record_of(r):
    """a PhotometricFrame as the dict above"""
    return dict(gain=tuple(r.gain), flags=int(r.flags), count=int(r.count), sum=tuple(r.sum), target=tuple(r.target))


# ---- the inputs of the GPU test -------------------------------------------------------------------------

def response(kind="bump"):
    """3 x 256 uint16, another curve per channel (so that an exchange of channels shows); "max": all 65535"""
    if kind == "max":
        return np.full((3, 256), 65535, np.uint16)
    b = np.arange(256, dtype=np.int64)
    return np.stack([np.clip(b * 256 + (c + 1) * ((b * (255 - b)) >> 1) + 37 * c, 0, 65535) for c in range(3)]).astype(np.uint16)


def vignette(w, h):
    """Q12 gains growing from the centre, no symmetry in x and y (so that rows of another length show)"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    cx, cy = w // 2, h // 2
    r2 = (xx - cx) ** 2 + 3 * (yy - cy) ** 2
    return (4096 + (r2 * 3000) // (cx * cx + 3 * cy * cy + 1) + (xx * 7 + yy * 13) % 5).astype(np.uint16)


def image(w, h, kind, seed=5, min_count=1, lo=8, hi=247):
    """random: uniform bytes (some outside the window, some at its ends); dark: those times 0.5; none: no pixel counts
    (every pixel has a channel outside the window); exact / below: exactly min_count / min_count - 1 pixels count, each
    with a channel at `lo` and one at `hi`"""
    rng = np.random.RandomState(seed + 31 * w + h)
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "dark":
        img = (img >> 1).astype(np.uint8)
        img[0, 0] = (lo, lo + 1, hi >> 1)
    elif kind in ("none", "exact", "below"):
        out = rng.randint(0, 2, (h, w)).astype(bool)
        img[..., 0] = np.where(out, rng.randint(hi + 1, 256, (h, w)), rng.randint(0, max(lo, 1), (h, w)))
        n = 0 if kind == "none" else min(min_count - (kind == "below"), w * h)
        flat = img.reshape(-1, 3)
        for p in rng.permutation(w * h)[:n]:
            flat[p] = (lo, hi, rng.randint(lo, hi + 1))
    return img


TARGET = (40000, 32000, 20000)
COMBOS = tuple(
    [("tables %d" % t, setting(t)) for t in (1, 2, 3)] +
    [("gain, tables %d" % t, setting(GAIN | t, gain_min=1000, gain_max=20000)) for t in (0, 1, 2, 3)] +
    [("auto %s, tables %d, per_channel %d" % (name, t, pc), setting(AUTO | t, per_channel=pc, target=tg, min_count=3,
                                                                    gain_min=3500, gain_max=6000))
     for t in (0, 1, 2, 3) for pc in (0, 1) for name, tg in (("lock", (0, 0, 0)), ("target", TARGET))])
GAINS = ((5851, 4096, 3000), (65535, 1, 19999))


def cases(sizes=SIZES):
    """(name, w, h, setting, response, vignette, gains_q12, image kind) of every stand-alone run of the GPU test"""
    for w, h in sizes:
        for name, s in COMBOS:
            resp = response() if s[0] & RESPONSE else None
            vig = vignette(w, h) if s[0] & VIGNETTE else None
            if s[0] & AUTO:
                kinds = ("random", "dark", "none", "exact", "below")
                for kind in kinds:
                    yield (name, w, h, s, resp, vig, None, kind)
            elif s[0] & GAIN:
                for g in GAINS:
                    yield (name, w, h, s, resp, vig, g, "random")
            else:
                yield (name, w, h, s, resp, vig, None, "random")


def case_image(case):
    _, w, h, s, _, _, _, kind = case
    return image(w, h, kind, min_count=s[3], lo=s[1], hi=s[2])


def case_frame(case, **steps):
    _, w, h, s, resp, vig, gains, _ = case
    return frame(case_image(case), s, resp, vig, gains, **steps)[:2]


def darkened(img, factor):
    return np.floor(img.astype(np.float64) * factor + 0.5).astype(np.uint8)


def auto_sequence(w, h, seed=72):
    """the frames of the lock test: one picture, its third frame darkened to 0.6, its fifth without a counted pixel; the
    same again behind a rearm"""
    rng = np.random.RandomState(seed)
    base = rng.randint(30, 200, (h, w, 3)).astype(np.uint8)
    frames = [base, darkened(base, 0.9), darkened(base, 0.6), base, np.full((h, w, 3), 255, np.uint8), darkened(base, 0.8)]
    return frames


def run_sequence(frames, s, response=None, vignette=None, rearm_at=(), **steps):
    state, out = OPEN, []
    for i, img in enumerate(frames):
        o, rec, state = frame(img, s, response, vignette, None, state, rearm=i in rearm_at, **steps)[:3]
        out.append((o, rec))
    return out
