"""Reference (test infrastructure only): the layout a cloud has in device memory after its hand-over
(csrc/cvo_cloud.hip: bounding box, 30-bit Morton keys, a stable sort, packed rows, bounding spheres of the
64-point runs, padding rows), restated in numpy -- every step in the type the device
uses, nothing shared with the library.  tests/test_cloud_layout_cpu.py holds this module to definitions,
tests/test_gpu_cloud_layout.py holds the device to this module, bit for bit.

Float arrays are compared through .view(np.uint32): the padding rows are NaN on purpose."""
import numpy as np

SEG = 64          # rows of a run (one bounding sphere each)
BUCKET = 256      # rows are padded to a multiple of this
F32 = np.float32
QNAN_BITS = np.uint32(0x7FC00000)


def bounding_box(xyz):
    """(lo[3], hi[3]) in float32."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    return xyz.min(0), xyz.max(0)


def spread_bits(v):
    """Bit b of the 10-bit value goes to bit 3 b."""
    v = np.asarray(v, np.uint32)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def quantise(xyz, lo, hi):
    """The 10-bit cell of every point on every axis: uint32 n x 3."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    q = np.zeros(xyz.shape, np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            ext = F32(hi[a] - lo[a])
            inv = F32(1023.0) / ext if (ext > F32(0.0) and ext <= F32(3.4e38)) else F32(0.0)
            f = ((xyz[:, a] - lo[a]).astype(F32) * inv).astype(F32)
            f = np.where(f >= F32(0.0), f, F32(0.0))      # (not f >= 0, NaN included)
            f = np.where(f > F32(1023.0), F32(1023.0), f)
            q[:, a] = f.astype(np.uint32)                 # truncation
    return q


def morton_keys(xyz, lo, hi):
    q = quantise(xyz, lo, hi)
    return spread_bits(q[:, 0]) | (spread_bits(q[:, 1]) << np.uint32(1)) | (spread_bits(q[:, 2]) << np.uint32(2))


def run_spheres(pos_live):
    """(centre xyz, radius) float32 [runs, 4] of the runs of SEG rows of pos_live (n x >=3 float32)."""
    p = np.asarray(pos_live, F32)[:, :3]
    n = p.shape[0]
    starts = np.arange(0, n, SEG)
    lo = np.minimum.reduceat(p, starts, axis=0)
    hi = np.maximum.reduceat(p, starts, axis=0)
    c = (0.5 * (lo.astype(np.float64) + hi.astype(np.float64))).astype(F32)
    d = p.astype(np.float64) - c.astype(np.float64)[np.arange(n) // SEG]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(over="ignore"):
        r = (np.sqrt(np.maximum.reduceat(d2, starts)) * 1.00001 + 1e-6).astype(F32)
    return np.concatenate([c, r[:, None]], axis=1)


def layout(xyz, feat, colmajor, pad_axis):
    """xyz n x 3, feat n x 5 (or 5 x n with colmajor), n >= 1 -> rows, pos[rows, 4], feat8[rows, 8],
    seg[ceil(rows / 64), 4], bbox[6], order[n]."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n = xyz.shape[0]
    feat = np.asarray(feat, F32)
    feat = feat.reshape(5, n).T if colmajor else feat.reshape(n, 5)
    lo, hi = bounding_box(xyz)
    keys = morton_keys(xyz, lo, hi)
    order = np.argsort(keys, kind="stable")
    rows = (n + BUCKET - 1) // BUCKET * BUCKET
    pos = np.zeros((rows, 4), F32)
    feat8 = np.zeros((rows, 8), F32)
    seg = np.zeros((rows // SEG, 4), F32)
    pos[:n, :3] = xyz[order]
    pos[:n, 3] = feat[order, 4]
    feat8[:n, :5] = feat[order]
    feat8[:n, 5] = order.astype(np.int32).view(F32)
    live_runs = (n + SEG - 1) // SEG
    seg[:live_runs] = run_spheres(pos[:n])
    # padding rows: far away along pad_axis, 16 m apart, NaN features, index -1
    with np.errstate(over="ignore"):
        centre = (F32(0.5) * (lo + hi).astype(F32)).astype(F32)
    k = np.arange(rows - n)
    off = (F32(1.0e4) + (F32(16.0) * k.astype(F32)).astype(F32)).astype(F32)
    pos[n:, :3] = centre
    pos[n:, pad_axis] = (centre[pad_axis] + off).astype(F32)
    pos.view(np.uint32)[n:, 3] = QNAN_BITS
    feat8.view(np.uint32)[n:, :5] = QNAN_BITS
    feat8[n:, 5] = np.full(rows - n, -1, np.int32).view(F32)
    for g in range(live_runs, rows // SEG):   # runs of padding only
        first = pos[g * SEG, :3].copy()
        first[pad_axis] = F32(first[pad_axis] + F32(8.0 * SEG))
        first[1 - pad_axis] = F32(first[1 - pad_axis] + F32(0.0))
        seg[g, :3] = first
        seg[g, 3] = F32(8.5 * SEG)
    return rows, pos, feat8, seg, np.concatenate([lo, hi]).astype(F32), order
