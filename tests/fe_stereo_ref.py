"""A numpy restatement of the front end's stereo contract (include/cvo_frontend.h, at cvo_fe_stereo),
stage by stage: grey, census, S, dL, dR, flags, q, the table, the plane.  Everything but the table is integer
arithmetic; the table is float64 on floats widened exactly.  The order of operations below is the contract;
the kernels of csrc/cvo_stereo.hip repeat it.

Settings here are a dict with the members of cvo_fe_stereo (without pad_).  Also here: the synthetic pairs and
the cases the tests share, CASES and EDGE_CASES."""
import numpy as np

UNIQUE, LR, MIN, DEPTH = 1, 2, 4, 8
BIG = 1 << 20                       # above every S and every L_r
_POP16 = np.array([bin(v).count("1") for v in range(1 << 16)], np.uint8)


def make_stereo(baseline=0.25, max_disp=32, min_disp=1, p1=8, p2=32, uniqueness=10, lr_max=1):
    """the default settings of the shared cases"""
    return dict(baseline=baseline, max_disp=max_disp, min_disp=min_disp, p1=p1, p2=p2, uniqueness=uniqueness, lr_max=lr_max)


def to_struct(F, st):
    """The settings as the package's Stereo."""
    return None if st is None else F.Stereo(**st)


# ---- the contract, stage by stage ------------------------------------------------------------------

def grey(img):
    """1: h x w x 3 uint8 -> h x w uint8"""
    c = np.asarray(img).astype(np.int64)
    return ((c[:, :, 0] * 4899 + c[:, :, 1] * 9617 + c[:, :, 2] * 1868 + 8192) >> 14).astype(np.uint8)


def census(g):
    """2: h x w uint8 -> h x w uint64, 62 bits"""
    g = np.asarray(g)
    h, w = g.shape
    P = np.pad(g, ((3, 3), (4, 4)), mode="edge").astype(np.int64)   # the neighbour's coordinates clamped to the image
    centre = g.astype(np.int64)
    c = np.zeros((h, w), np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            n = P[3 + dy:3 + dy + h, 4 + dx:4 + dx + w]
            c = (c << np.uint64(1)) | (n < centre).astype(np.uint64)
    return c


def popcount(x):
    x = np.ascontiguousarray(x, np.uint64)
    return _POP16[x.view(np.uint16).reshape(x.shape + (4,))].sum(axis=-1, dtype=np.int64)


def cost(cl, cr, D):
    """3: C h x w x D int64"""
    h, w = cl.shape
    C = np.full((h, w, D), 64, np.int64)
    for d in range(min(D, w)):
        C[:, d:, d] = popcount(cl[:, d:] ^ cr[:, :w - d])
    return C


def _scan(Cs, p1, p2):
    """the recurrence of 4 along axis 0 of Cs (steps x lines x D): the L_r of every step"""
    out = np.empty_like(Cs)
    L = Cs[0].copy()
    out[0] = L
    for t in range(1, Cs.shape[0]):
        m = L.min(axis=1, keepdims=True)
        below = np.full_like(L, BIG)
        below[:, 1:] = L[:, :-1] + p1
        above = np.full_like(L, BIG)
        above[:, :-1] = L[:, 1:] + p1
        L = Cs[t] + np.minimum(np.minimum(L, m + p2), np.minimum(below, above)) - m
        out[t] = L
    return out


def path_sums(C, p1, p2):
    """4: S h x w x D uint16"""
    Ct = C.transpose(1, 0, 2)                              # steps over x, lines over y
    S = _scan(Ct, p1, p2).transpose(1, 0, 2)               # left to right
    S = S + _scan(Ct[::-1], p1, p2)[::-1].transpose(1, 0, 2)   # right to left
    S = S + _scan(C, p1, p2)                               # top to bottom
    S = S + _scan(C[::-1], p1, p2)[::-1]                   # bottom to top
    assert S.max() <= 4 * (64 + 255)
    return S.astype(np.uint16)


def path_sums_loops(C, p1, p2):
    """4 again, one pixel and one d at a time"""
    h, w, D = C.shape
    S = np.zeros((h, w, D), np.int64)
    for (ry, rx) in ((0, 1), (0, -1), (1, 0), (-1, 0)):
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
        S += L
    return S.astype(np.uint16)


def winners(S):
    """5: (d*, S1), the smallest d on ties"""
    S = S.astype(np.int64)
    ds = S.argmin(axis=2)
    return ds, np.take_along_axis(S, ds[:, :, None], 2)[:, :, 0]


def not_unique(S, ds, S1, uniqueness):
    """6"""
    S = S.astype(np.int64)
    D = S.shape[2]
    far = np.abs(np.arange(D)[None, None, :] - ds[:, :, None]) > 1
    S2 = np.where(far, S, BIG).min(axis=2)
    return far.any(axis=2) & (S2 * (100 - uniqueness) < S1 * 100)


def right_map(S):
    """7: dR"""
    S = S.astype(np.int64)
    h, w, D = S.shape
    SR = np.full((h, w, D), BIG, np.int64)
    for d in range(min(D, w)):
        SR[:, :w - d, d] = S[:, d:, d]
    return SR.argmin(axis=2)


def lr_fails(ds, dR, lr_max):
    h, w = ds.shape
    if lr_max < 0:
        return np.zeros((h, w), bool)
    x = np.arange(w)[None, :]
    xr = x - ds
    there = dR[np.arange(h)[:, None], np.clip(xr, 0, w - 1)]
    return (xr < 0) | (np.abs(there - ds) > lr_max)


def subpixel(S, ds, S1):
    """8: q"""
    S = S.astype(np.int64)
    D = S.shape[2]
    Sm = np.take_along_axis(S, np.clip(ds - 1, 0, D - 1)[:, :, None], 2)[:, :, 0]
    Sp = np.take_along_axis(S, np.clip(ds + 1, 0, D - 1)[:, :, None], 2)[:, :, 0]
    den = Sm + Sp - 2 * S1
    ok = (ds > 0) & (ds < D - 1) & (den > 0)
    off = np.where(ok, ((Sm - Sp) * 16 + den) // np.where(ok, 2 * den, 1), 0)   # (// floors)
    assert off.min() >= -8 and off.max() <= 8
    return 16 * ds + off


def depth_table(st, fx, depth_scale):
    """9: U(q), q = 0 .. 16 D - 1, uint16"""
    f = np.float32
    num = ((np.float64(f(fx)) * np.float64(f(st["baseline"]))) * np.float64(f(depth_scale))) * np.float64(16.0)
    n = 16 * st["max_disp"]
    U = np.zeros(n, np.float64)
    q = np.arange(max(16 * st["min_disp"], 1), n)
    U[q] = np.rint(num / q.astype(np.float64))
    U[(U < 1.0) | (U > 65535.0)] = 0.0
    return U.astype(np.uint16)


def match(left, right, st, fx, depth_scale):
    """Every plane of a stereo frame, by name."""
    D = st["max_disp"]
    gl, gr = grey(left), grey(right)
    cl, cr = census(gl), census(gr)
    S = path_sums(cost(cl, cr, D), st["p1"], st["p2"])
    return dict(decide(S, st, fx, depth_scale), gray_l=gl, gray_r=gr, census_l=cl, census_r=cr)


def decide(S, st, fx, depth_scale, winners=winners, not_unique=not_unique, right_map=right_map, subpixel=subpixel):
    """5 to 10: the planes behind the cost sums.  (The keywords put another form of one stage in its place: the
    mutants of tests/fe_stereo_mutants.py.)"""
    ds, S1 = winners(S)
    dR = right_map(S)
    q = subpixel(S, ds, S1)
    U = depth_table(st, fx, depth_scale)
    flags = np.zeros(ds.shape, np.int64)
    flags |= np.where(not_unique(S, ds, S1, st["uniqueness"]), UNIQUE, 0)
    flags |= np.where(lr_fails(ds, dR, st["lr_max"]), LR, 0)
    flags |= np.where(q < 16 * st["min_disp"], MIN, 0)
    flags = np.where((flags == 0) & (U[q] == 0), DEPTH, flags).astype(np.uint8)
    keep = flags == 0
    return dict(sum=S, dL=ds, dR=dR, q=q, table=U, flags=flags,
                disparity=np.where(keep, q, 0).astype(np.uint16), depth=np.where(keep, U[q], 0).astype(np.uint16))


# ---- the pairs -----------------------------------------------------------------------------------

PAD = 80          # columns of texture to the left of the right image: room for the largest disparity of a scene
FX, SCALE = 718.856, 2000.0     # row 4 of the camera table ("kitti 15"), the camera of every case: dataset_seq 4
SEQ = 4


def texture(h, w, seed):
    """uniform random bytes, smoothed once with [1 2 1] / 4 in both directions and stretched to 0..255; three channels"""
    rng = np.random.Generator(np.random.PCG64(3000 + seed))
    t = rng.integers(0, 256, (h + 2, w + 2, 3)).astype(np.float64)
    t = (t[:, :-2] + 2.0 * t[:, 1:-1] + t[:, 2:]) / 4.0
    t = (t[:-2] + 2.0 * t[1:-1] + t[2:]) / 4.0
    lo, hi = t.min(), t.max()
    return (t - lo) * (255.0 / (hi - lo))


def disparity_map(w, h, box=15.0, back=6.0):
    """`back` on the background, `box` inside the central box, a ramp from 4 to 9 across the top h / 6 rows"""
    disp = np.full((h, w), back)
    disp[h // 4:3 * h // 4, w // 3:2 * w // 3] = box
    disp[:h // 6, :] = 4.0 + 5.0 * np.arange(w)[None, :] / (w - 1)
    return disp


def pair(w, h, seed, box=15.0, back=6.0, pad=PAD):
    """(left, right, disp): the right image is a window of the texture, the left one the right one resampled at
    x - disp(x, y), bilinear and rounded; `pad` columns of texture lie to the left of the right image"""
    tex = texture(h, w + pad, seed)
    disp = disparity_map(w, h, box, back)
    assert disp.max() + 1 < pad
    xs = pad + np.arange(w)[None, :] - disp
    x0 = np.floor(xs).astype(np.int64)
    a = (xs - x0)[:, :, None]
    rows = np.arange(h)[:, None]
    left = (1.0 - a) * tex[rows, x0] + a * tex[rows, x0 + 1]
    right = tex[:, pad:pad + w]
    as_bytes = lambda t: np.ascontiguousarray(np.clip(np.rint(t), 0, 255).astype(np.uint8))
    return as_bytes(left), as_bytes(right), disp


def regions(w, h, margin=6):
    """(box interior, lower background, ramp): bool planes, the first two at least `margin` pixels inside"""
    box = np.zeros((h, w), bool)
    box[h // 4 + margin:3 * h // 4 - margin, w // 3 + margin:2 * w // 3 - margin] = True
    near_box = np.zeros((h, w), bool)
    near_box[max(h // 4 - margin, 0):3 * h // 4 + margin, max(w // 3 - margin, 0):2 * w // 3 + margin] = True
    back = np.zeros((h, w), bool)
    back[h // 6 + margin:h - margin, margin:w - margin] = True
    back &= ~near_box
    ramp = np.zeros((h, w), bool)
    ramp[:h // 6, :] = True
    return box, back, ramp


SIZES = [(64, 64, 32), (96, 64, 32), (127, 193, 48)]       # width, height, max_disp
SEEDS = (81, 82, 83)
# name: (width, height, seed, settings, the box's disparity; None: a texture-free pair, the background's disparity)
CASES = {}
for _w, _h, _D in SIZES:
    for _seed in SEEDS:
        CASES["default-%dx%d-%d" % (_w, _h, _seed)] = (_w, _h, _seed, make_stereo(max_disp=_D), 15.0, 6.0)
CASES["d128"] = (160, 64, 81, make_stereo(max_disp=128), 70.0, 6.0)
CASES["uniqueness0"] = (96, 64, 82, make_stereo(uniqueness=0), 15.0, 6.0)
CASES["lr-off"] = (96, 64, 82, make_stereo(lr_max=-1), 15.0, 6.0)
# (under min_disp 8 a background at 6 has no depth by design and a sixth of the image would be left: this case's
# background lies at 10, and the rule decides on the ramp below 8 and at the left border)
CASES["min8"] = (96, 64, 82, make_stereo(min_disp=8), 15.0, 10.0)
CASES["flat"] = (96, 64, 0, make_stereo(), None, None)
DEFAULTS = [n for n in CASES if n.startswith("default-")]


def case_inputs(name):
    """(settings, left, right, disp or None) of a case"""
    w, h, seed, st, box, back = CASES[name]
    if box is None:
        flat = np.empty((h, w, 3), np.uint8)
        flat[:] = (90, 140, 30)
        return st, flat, flat.copy(), None
    left, right, disp = pair(w, h, seed, box, back)
    return st, left, right, disp


_DONE = {}


def case_planes(name):
    """match() of a case, computed once and left unchanged"""
    if name not in _DONE:
        st, left, right, _ = case_inputs(name)
        out = match(left, right, st, FX, SCALE)
        for a in out.values():
            a.setflags(write=False)
        _DONE[name] = out
    return _DONE[name]


# ---- the edge cases: the seam between the two disparities of a lane, the ends of D, settings at the edge of what
# cvo_fe_check_stereo accepts, hostile images.  A table of its own beside CASES; what each one is for is asserted
# in tests/test_fe_stereo_cpu.py ---------------------------------------------------------------------------------

EDGE_PAD = 140         # room for a disparity of 127 and the ramp's reach
EDGE_BASELINE = 0.54   # 388 m px at FX: every disparity from 12 pixels up has a depth at 2000 units per metre
# uniqueness 0 and lr_max -1 switch both tests off: the disparity plane then shows q wherever there is a depth
_OPEN = dict(baseline=EDGE_BASELINE, uniqueness=0, lr_max=-1)
_LR0 = dict(baseline=EDGE_BASELINE, lr_max=0)
# name: (width, height, settings, scene).  Scenes: ("pair", seed, box, back, pad) is pair(); ("noise", seed) two
# independent planes of uniform random bytes; ("stripes",) vertical stripes of period 8, ("checker",) a one-pixel
# checkerboard and ("same", seed) a texture, each the same in both images; ("saturated",) left all 255, right all 0;
# ("tail", seed, k) is "same" with the last k columns of the left image replaced by uniform random bytes
EDGE_CASES = {
    "seam-128": (192, 64, make_stereo(max_disp=128, **_OPEN), ("pair", 81, 63.5, 6.0, EDGE_PAD)),
    "seam-72": (192, 64, make_stereo(max_disp=72, **_OPEN), ("pair", 81, 64.5, 6.0, EDGE_PAD)),
    "seam-back": (192, 64, make_stereo(max_disp=128, **_OPEN), ("pair", 81, 64.0, 62.0, EDGE_PAD)),
    "full-64": (192, 64, make_stereo(max_disp=64, **_OPEN), ("pair", 81, 62.5, 6.0, EDGE_PAD)),
    "top-128": (320, 64, make_stereo(max_disp=128, **_OPEN), ("pair", 81, 126.5, 120.0, EDGE_PAD)),
    # (a background at 3 pixels has a depth below 0.137 m of baseline only)
    "d8": (64, 64, make_stereo(max_disp=8, **dict(_OPEN, baseline=0.1)), ("pair", 81, 6.5, 3.0, EDGE_PAD)),
    "d120": (288, 64, make_stereo(max_disp=120, **_OPEN), ("pair", 81, 100.5, 70.0, EDGE_PAD)),
    "narrow": (64, 64, make_stereo(max_disp=128, **_OPEN), ("pair", 81, 15.0, 6.0, EDGE_PAD)),
    "wide": (1241, 64, make_stereo(max_disp=128, **_OPEN), ("pair", 81, 70.0, 6.0, EDGE_PAD)),
    # the seam scenes under the default uniqueness and lr_max 0: LR turns on the exact dR
    "seam-128-lr0": (192, 64, make_stereo(max_disp=128, **_LR0), ("pair", 81, 63.5, 6.0, EDGE_PAD)),
    "seam-72-lr0": (192, 64, make_stereo(max_disp=72, **_LR0), ("pair", 81, 64.5, 6.0, EDGE_PAD)),
    "seam-back-lr0": (192, 64, make_stereo(max_disp=128, **_LR0), ("pair", 81, 64.0, 62.0, EDGE_PAD)),
    # settings at the edge of what is accepted, on the pair of default-96x64-82
    "p255": (96, 64, make_stereo(p1=255, p2=255), ("pair", 82, 15.0, 6.0, PAD)),
    "p255-noise": (96, 64, make_stereo(p1=255, p2=255), ("noise", 85)),
    "p1": (96, 64, make_stereo(p1=1, p2=1), ("pair", 82, 15.0, 6.0, PAD)),
    "u99-lr8": (96, 64, make_stereo(uniqueness=99, lr_max=8), ("pair", 82, 15.0, 6.0, PAD)),
    "lr0": (96, 64, make_stereo(lr_max=0), ("pair", 82, 15.0, 6.0, PAD)),
    "min200": (96, 64, make_stereo(min_disp=200), ("pair", 82, 15.0, 6.0, PAD)),
    # (FX * 1e-6 * SCALE * 16 = 23: the table is 1 up to q = 46 and 0 from there, so under min_disp 3 it is all zero)
    "baseline1e-6": (96, 64, make_stereo(baseline=1e-6), ("pair", 82, 15.0, 6.0, PAD)),
    "baseline1e-6-min3": (96, 64, make_stereo(baseline=1e-6, min_disp=3), ("pair", 82, 15.0, 6.0, PAD)),
    # hostile images under the default settings
    "noise": (96, 64, make_stereo(), ("noise", 85)),
    "stripes": (96, 64, make_stereo(), ("stripes",)),
    "checker": (96, 64, make_stereo(), ("checker",)),
    "saturated": (96, 64, make_stereo(), ("saturated",)),
    "same": (96, 64, make_stereo(), ("same", 82)),
    # the right map's x + d < w: the last two columns of the left image match nothing, so right pixels there have
    # only costly candidates inside the row, and the row below begins with cheap ones (see the CPU test)
    "tail": (96, 64, make_stereo(p2=255, lr_max=0), ("tail", 82, 2)),
}
STRIPE = (40, 90, 200, 250, 160, 120, 60, 10)     # one period of the stripes, every channel


def edge_inputs(name):
    """(settings, left, right, disp or None) of an edge case"""
    w, h, st, scene = EDGE_CASES[name]
    kind = scene[0]
    if kind == "pair":
        left, right, disp = pair(w, h, *scene[1:4], pad=scene[4])
        return st, left, right, disp
    if kind == "noise":
        rng = np.random.Generator(np.random.PCG64(3000 + scene[1]))
        left, right = (rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2))
    elif kind == "saturated":
        left, right = np.full((h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8)
    else:
        if kind == "stripes":
            plane = np.broadcast_to(np.array(STRIPE)[np.arange(w) % 8][None, :, None], (h, w, 3))
        elif kind == "checker":
            plane = np.broadcast_to((255 * ((np.arange(w)[None, :] + np.arange(h)[:, None]) % 2))[:, :, None], (h, w, 3))
        else:
            plane = np.rint(texture(h, w, scene[1]))
        left = np.ascontiguousarray(plane.astype(np.uint8))
        right = left.copy()
        if kind == "tail":
            rng = np.random.Generator(np.random.PCG64(4000 + scene[1]))
            left[:, w - scene[2]:] = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)[:, w - scene[2]:]
    return st, left, right, None


def edge_planes(name):
    """match() of an edge case, computed once and left unchanged"""
    key = ("edge", name)
    if key not in _DONE:
        st, left, right, _ = edge_inputs(name)
        out = match(left, right, st, FX, SCALE)
        for a in out.values():
            a.setflags(write=False)
        _DONE[key] = out
    return _DONE[key]


def bad_stereos():
    """Settings cvo_fe_check_stereo refuses, every member in turn (pad_ included)"""
    nan, inf = float("nan"), float("inf")
    good = make_stereo()
    return [dict(good, **{k: v}) for k, v in (
        ("baseline", 0.0), ("baseline", -0.5), ("baseline", nan), ("baseline", inf),
        ("max_disp", 0), ("max_disp", 4), ("max_disp", 36), ("max_disp", 136), ("max_disp", -8),
        ("min_disp", 0), ("min_disp", -1), ("p1", 0), ("p1", 33), ("p2", 256), ("p2", 7),
        ("uniqueness", -1), ("uniqueness", 100), ("lr_max", -2), ("lr_max", 9), ("pad_", 1))]


def good_stereos():
    """... and settings at the edge of what it accepts"""
    return [make_stereo(), make_stereo(max_disp=8), make_stereo(max_disp=128), make_stereo(p1=1, p2=1),
            make_stereo(p1=255, p2=255), make_stereo(uniqueness=0), make_stereo(uniqueness=99), make_stereo(lr_max=-1),
            make_stereo(lr_max=8), make_stereo(min_disp=200), make_stereo(baseline=1e-6)]
