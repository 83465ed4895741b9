"""A numpy restatement of the front end's gate contract (include/cvo_frontend.h, at
cvo_fe_depth_gate): integer planes and float32 scalars (numpy's float32 multiplication and
division are single, correctly rounded operations and nothing is contracted).  The order of
operations below is the contract; k_fe_depth_gate of csrc/cvo_frontend.hip repeats it.

A gate here is a dict with the members of cvo_fe_depth_gate (without pad_), or None: no gate.
Also here: the scenes, the masks and the (scene, gate) cases the tests share."""
import numpy as np

MASKED, RANGE, JUMP = 1, 2, 4
TILE = (64, 16)     # k_fe_depth_gate's tile, width x height: where the seam scene puts its steps
SCALE = 5000.0      # depth units per metre of the table's row 1 and of every scene here

NEIGHBOURS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def make_gate(min_range=0.0, max_range=0.0, jump_rel=0.0, grow=0, hole_border=0):
    return dict(min_range=min_range, max_range=max_range, jump_rel=jump_rel, grow=grow, hole_border=hole_border)


def to_struct(F, gate):
    """The gate as the package's DepthGate."""
    return None if gate is None else F.DepthGate(**gate)


def _shifted(P, dy, dx, r, h, w):
    """The plane padded by r on every side, seen from (dy, dx) away"""
    return P[r + dy:r + dy + h, r + dx:r + dx + w]


def jump_marks(U, jump_rel, hole_border):
    """J: bool h x w.  Neighbours outside the image never mark; J = 0 where U == 0."""
    U = np.asarray(U).astype(np.int64)
    h, w = U.shape
    f = np.float32
    P = np.full((h + 2, w + 2), -1, np.int64)     # -1: outside the image
    P[1:-1, 1:-1] = U
    J = np.zeros((h, w), bool)
    for dy, dx in NEIGHBOURS:
        q = _shifted(P, dy, dx, 1, h, w)
        if hole_border:
            J |= q == 0
        if f(jump_rel) > 0:
            m = np.minimum(U, q)
            D = np.maximum(U, q) - m
            jump = D.astype(f) > f(jump_rel) * m.astype(f)
            assert (f(jump_rel) * m.astype(f)).dtype == f
            J |= (q > 0) & jump
    return J & (U != 0)


def near(J, grow):
    """some q inside the image with max(|dx|, |dy|) <= grow has J(q)"""
    h, w = J.shape
    g = int(grow)
    P = np.zeros((h + 2 * g, w + 2 * g), bool)
    P[g:g + h, g:g + w] = J
    out = np.zeros((h, w), bool)
    for dy in range(-g, g + 1):
        for dx in range(-g, g + 1):
            out |= _shifted(P, dy, dx, g, h, w)
    return out


def out_of_range(U, min_range, max_range, scale):
    f = np.float32
    z = np.asarray(U).astype(f) / f(scale)
    assert z.dtype == f
    out = np.zeros(z.shape, bool)
    if f(min_range) > 0:
        out |= z < f(min_range)
    if f(max_range) > 0:
        out |= z > f(max_range)
    return out


def masked_plain(mask):
    return np.asarray(mask) != 0


def masked_through_map(mask, qu, qv):
    """The mask through a rectification map by the depth rule: outside the image counts as masked."""
    mask = np.asarray(mask)
    h, w = mask.shape
    xn = (qu.astype(np.int64) + 16) >> 5
    yn = (qv.astype(np.int64) + 16) >> 5
    inside = (xn >= 0) & (xn < w) & (yn >= 0) & (yn < h)
    return ~inside | (mask[np.clip(yn, 0, h - 1), np.clip(xn, 0, w - 1)] != 0)


def rule_planes(U, gate, scale, mask=None, qu=None, qv=None):
    """(masked, range, near a jump): bool planes, each 0 where U == 0"""
    U = np.asarray(U)
    assert U.dtype == np.uint16
    valid = U != 0
    zero = np.zeros(U.shape, bool)
    m = zero if mask is None else (masked_plain(mask) if qu is None else masked_through_map(mask, qu, qv))
    if gate is None:
        return m & valid, zero, zero
    r = out_of_range(U, gate["min_range"], gate["max_range"], scale)
    n = near(jump_marks(U, gate["jump_rel"], gate["hole_border"]), gate["grow"])
    return m & valid, r & valid, n & valid


def gate(U, gate, scale, mask=None, qu=None, qv=None):
    """(depth uint16, flags uint8) of the contract"""
    m, r, n = rule_planes(U, gate, scale, mask, qu, qv)
    flags = (m * MASKED + r * RANGE + n * JUMP).astype(np.uint8)
    return np.where(flags != 0, 0, U).astype(np.uint16), flags


# ---- scenes, masks and cases --------------------------------------------------------------------

def _data():
    from __graft_entry__ import load_package
    return load_package().data


def frame(w, h, seed):
    """The colour image that goes with gate_scene(w, h, seed)"""
    return _data().synthetic_rgbd_frame(width=w, height=h, seed=seed, texture=1.0, holes=0.0)[0]


def _put_holes(dep, holes, rng):
    h, w = dep.shape
    if holes == "random":
        dep[rng.random((h, w)) < 0.02] = 0
    elif holes == "blocks":
        dep[h // 3:h // 3 + 6, w // 5:w // 5 + 9] = 0
        dep[2 * h // 3:2 * h // 3 + 5, 3 * w // 5:3 * w // 5 + 7] = 0
    else:
        assert holes is None


def gate_scene(w, h, seed, holes="random"):
    """The slanted plane of data.synthetic_rgbd_frame (1.2 - 2.0 m at 5000 units per metre) with a few dozen
    random boxes of random depth inside the range, a near box at 0.7 m touching the top-left corner, a far
    strip at 5.5 m along the bottom-right border, a 3 x 3 bump of +6 % in the interior, and holes: 2 % random
    pixels ("random"), two solid blocks ("blocks") or none (None)."""
    dep = _data().synthetic_rgbd_frame(width=w, height=h, seed=seed, texture=1.0, holes=0.0)[1].astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    for _ in range(24):
        bw, bh = rng.integers(2, max(4, w // 10), endpoint=True), rng.integers(2, max(4, h // 10), endpoint=True)
        x, y = rng.integers(0, w - bw, endpoint=True), rng.integers(0, h - bh, endpoint=True)
        dep[y:y + bh, x:x + bw] = int(rng.integers(4500, 19000))       # 0.9 - 3.8 m
    dep[0:h // 5, 0:w // 4] = 3500
    dep[h - h // 8:, w // 2:] = 27500
    cy, cx = h // 2, w // 2
    dep[cy - 1:cy + 2, cx - 1:cx + 2] = np.rint(dep[cy - 1:cy + 2, cx - 1:cx + 2] * 1.06).astype(np.int64)
    _put_holes(dep, holes, rng)
    return np.ascontiguousarray(dep.astype(np.uint16))


def seam_scene(w, h, seed):
    """Steps exactly on the seams of the kernel's 64 x 16 tiles and on all four image borders: boxes whose edges lie
    on x = 64 from either side and on y = 16, 32, 48; strips two pixels wide along each border; a block of holes
    across a seam."""
    tw, th = TILE
    dep = _data().synthetic_rgbd_frame(width=w, height=h, seed=seed, texture=1.0, holes=0.0)[1].astype(np.int64)
    dep[th:2 * th, tw - 24:tw] = 4600           # right edge on the seam x = 64, top and bottom on y = 16, 32
    dep[2 * th:3 * th, tw:tw + 26] = 12000      # left edge on x = 64 (cut by a 64-wide image), y = 32, 48
    dep[0:2, 10:30] = 15000                     # the four borders
    dep[20:40, 0:2] = 15000
    dep[h - 2:, 5:25] = 4700
    dep[30:50, w - 2:] = 4700
    dep[3 * th - 2:3 * th + 2, 8:20] = 0        # holes across y = 48
    if h > 4 * th:
        dep[5 * th:7 * th, 30:tw + 10] = 9000   # (the tall image: across x = 64, edges on y = 80, 112)
    return np.ascontiguousarray(dep.astype(np.uint16))


def mask_scene(w, h, seed):
    """A block in the interior, where the scenes are mostly plane, and 1 % random pixels; several non-zero values"""
    rng = np.random.Generator(np.random.PCG64(2000 + seed))
    m = np.zeros((h, w), np.uint8)
    m[h // 2 + 4:h // 2 + 14, w // 8:w // 8 + 17] = 255
    m[rng.random((h, w)) < 0.01] = 1
    m[h // 4, w // 2] = 7
    return m


SIZES = [(64, 64), (96, 64), (127, 193)]
SEEDS = (72, 73, 74)
FULL = make_gate(0.8, 4.0, 0.05)
# name: (gate, scene, holes, with a mask)
CASES = {
    "grow0": (dict(FULL, grow=0), "gate", "random", False),
    "grow1": (dict(FULL, grow=1), "gate", "random", False),
    "grow3": (dict(FULL, grow=3), "gate", "random", False),
    "jump": (make_gate(jump_rel=0.05, grow=1), "gate", "random", False),
    "range": (make_gate(0.8, 4.0), "gate", "random", False),
    "holes": (dict(FULL, grow=1, hole_border=1), "gate", "blocks", False),
    "mask": (None, "gate", "random", True),
    "mask+gate": (dict(FULL, grow=1), "gate", "random", True),
    "seams": (make_gate(jump_rel=0.05, grow=3, hole_border=1), "seam", None, False),
}


def case_inputs(name, w, h, seed):
    """(gate, U, mask or None) of a case"""
    g, kind, holes, with_mask = CASES[name]
    U = seam_scene(w, h, seed) if kind == "seam" else gate_scene(w, h, seed, holes)
    return g, U, (mask_scene(w, h, seed) if with_mask else None)


def bad_gates():
    """Gates cvo_fe_check_depth_gate refuses, one rule each (pad_ included)"""
    nan, inf = float("nan"), float("inf")
    good = dict(FULL, grow=1)
    out = [dict(good, **{k: v}) for k, v in (
        ("min_range", nan), ("max_range", inf), ("jump_rel", nan), ("min_range", -inf), ("jump_rel", -0.01),
        ("grow", -1), ("grow", 4), ("hole_border", 2), ("hole_border", -1), ("pad_", 1))]
    out.append(dict(good, min_range=2.0, max_range=1.0))
    out.append(dict(good, min_range=0.8, max_range=0.8))
    return out


def good_gates():
    """... and gates at the edge of what it accepts"""
    return [make_gate(), make_gate(-1.0, -2.0), make_gate(3.0, 0.0), make_gate(0.8, 0.80001), make_gate(0.0, 4.0, 0.0, 3, 1),
            make_gate(jump_rel=1e-6), make_gate(jump_rel=10.0, grow=3), dict(FULL, grow=1)]
