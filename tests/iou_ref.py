"""Float64 NumPy restatement of the rotated-box IoU of include/dal3.h (dal3_box_iou_*): test infrastructure, the oracle
the GPU kernels are held to. Boxes (.,7) [x, y, z, l, w, h, yaw].

Same definition, written independently of the kernel: a's corners are put into b's frame (centre difference first,
then the rotation by -yaw_b, the corners rotated by yaw_a - yaw_b), and the textbook Sutherland–Hodgman clip runs
against the four half-planes x <= l_b/2, -x <= l_b/2, y <= w_b/2, -y <= w_b/2 one after the other. To stay vectorised
over pairs, every step emits exactly two points per input vertex E (predecessor S):
    S in,  E in   ->  E, E
    S out, E in   ->  I, E        (I = the edge's crossing of the clip line)
    S in,  E out  ->  I, I
    S out, E out  ->  E', E'      (E' = E projected onto the clip line)
Repeated points and points on the clip line between an exit and the next entry add nothing to the shoelace sum, so
the area is that of the textbook polygon. 4 -> 8 -> 16 -> 32 -> 64 points.

Also: monte_carlo_bev(), an estimate of the BEV IoU by sampling, for checking this oracle itself, and fixture_pairs(),
the pairs tests/golden/iou_ref_pairs.npz holds the reference's IoU of.
"""
import importlib

import numpy as np

CHUNK = 1 << 16


def _clip(x, y, lim, axis, sign):
    """one half-plane  sign * coord <= lim  (coord = x if axis == 0 else y); x, y (P, V) -> (P, 2V)"""
    u, v = (x, y) if axis == 0 else (y, x)
    su, sv = np.roll(u, 1, axis=1), np.roll(v, 1, axis=1)                  # predecessor S of every vertex E
    e_in, s_in = sign * u <= lim, sign * su <= lim
    line = sign * lim                                                        # the clip line's coordinate
    du = u - su
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(e_in != s_in, (line - su) / np.where(du == 0, 1.0, du), 0.0)
    iu, iv = np.full_like(u, 0.0) + line, sv + t * (v - sv)
    pu = np.full_like(u, 0.0) + line                                         # E projected onto the line
    first_u = np.where(e_in, np.where(s_in, u, iu), np.where(s_in, iu, pu))
    first_v = np.where(e_in, np.where(s_in, v, iv), np.where(s_in, iv, v))
    second_u = np.where(e_in, u, first_u)
    second_v = np.where(e_in, v, first_v)
    ou = np.stack([first_u, second_u], axis=2).reshape(u.shape[0], -1)
    ov = np.stack([first_v, second_v], axis=2).reshape(u.shape[0], -1)
    return (ou, ov) if axis == 0 else (ov, ou)


def _paired(a, b):
    a = np.asarray(a, np.float64).reshape(-1, 7)
    b = np.asarray(b, np.float64).reshape(-1, 7)
    bad = ~(np.isfinite(a).all(1) & np.isfinite(b).all(1))
    a, b = np.where(bad[:, None], 0.0, a), np.where(bad[:, None], 0.0, b)
    la, wa, ha = (np.maximum(a[:, k], 0.0) for k in (3, 4, 5))
    lb, wb, hb = (np.maximum(b[:, k], 0.0) for k in (3, 4, 5))
    dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    cb, sb = np.cos(b[:, 6]), np.sin(b[:, 6])
    px, py = cb * dx + sb * dy, cb * dy - sb * dx
    rel = a[:, 6] - b[:, 6]
    cr, sr = np.cos(rel), np.sin(rel)
    ux, uy, vx, vy = cr * la / 2, sr * la / 2, -sr * wa / 2, cr * wa / 2
    x = np.stack([px + ux + vx, px - ux + vx, px - ux - vx, px + ux - vx], 1)
    y = np.stack([py + uy + vy, py - uy + vy, py - uy - vy, py + uy - vy], 1)
    for axis, sign, lim in ((0, 1.0, lb / 2), (0, -1.0, lb / 2), (1, 1.0, wb / 2), (1, -1.0, wb / 2)):
        x, y = _clip(x, y, lim[:, None], axis, sign)
    inter = 0.5 * (x * np.roll(y, -1, axis=1) - np.roll(x, -1, axis=1) * y).sum(1)
    area_a, area_b = la * wa, lb * wb
    inter = np.clip(inter, 0.0, np.minimum(area_a, area_b))
    union = area_a + area_b - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        bev = np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)
        dz = a[:, 2] - b[:, 2]
        zo = np.maximum(np.minimum(dz + ha / 2, hb / 2) - np.maximum(dz - ha / 2, -hb / 2), 0.0)
        i3 = inter * zo
        u3 = area_a * ha + area_b * hb - i3
        v3 = np.where(u3 > 0, i3 / np.where(u3 > 0, u3, 1.0), 0.0)
    bev[bad], v3[bad] = np.nan, np.nan
    return bev, v3


def paired(a, b):
    """(n,7) vs (n,7), row k against row k -> (iou_bev (n,), iou_3d (n,)) float64"""
    a = np.asarray(a, np.float64).reshape(-1, 7)
    b = np.asarray(b, np.float64).reshape(-1, 7)
    out = [_paired(a[s:s + CHUNK], b[s:s + CHUNK]) for s in range(0, a.shape[0], CHUNK)]
    if not out:
        return np.zeros(0), np.zeros(0)
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def pairwise(a, b):
    """(n,7) x (m,7) -> (iou_bev (n,m), iou_3d (n,m)) float64. Only pairs whose bounding circles come within a margin
    of each other are clipped; every other pair is exactly 0 (its rectangles cannot meet)."""
    a = np.asarray(a, np.float64).reshape(-1, 7)
    b = np.asarray(b, np.float64).reshape(-1, 7)
    n, m = a.shape[0], b.shape[0]
    bev, v3 = np.zeros((n, m)), np.zeros((n, m))
    if n == 0 or m == 0:
        return bev, v3
    ra = np.hypot(np.maximum(a[:, 3], 0), np.maximum(a[:, 4], 0)) / 2
    rb = np.hypot(np.maximum(b[:, 3], 0), np.maximum(b[:, 4], 0)) / 2
    for s in range(0, n, 256):
        blk = a[s:s + 256]
        with np.errstate(invalid="ignore"):
            d2 = (blk[:, None, 0] - b[None, :, 0]) ** 2 + (blk[:, None, 1] - b[None, :, 1]) ** 2
            near = ~(d2 > ((ra[s:s + 256, None] + rb[None, :]) * (1 + 1e-9)) ** 2)      # NaN pairs included
        i, j = np.nonzero(near)
        if i.size:
            vb, vv = paired(blk[i], b[j])
            bev[s + i, j], v3[s + i, j] = vb, vv
    return bev, v3


def monte_carlo_bev(a, b, n_samples, seed=0):
    """BEV IoU of ONE pair by uniform sampling in a's rectangle: (estimate, its standard error)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    rng = np.random.default_rng(seed)
    u = (rng.random((n_samples, 2)) - 0.5) * a[3:5]
    ca, sa = np.cos(a[6]), np.sin(a[6])
    wx, wy = a[0] + ca * u[:, 0] - sa * u[:, 1], a[1] + sa * u[:, 0] + ca * u[:, 1]
    cb, sb = np.cos(b[6]), np.sin(b[6])
    dx, dy = wx - b[0], wy - b[1]
    bx, by = cb * dx + sb * dy, cb * dy - sb * dx
    p = np.mean((np.abs(bx) <= b[3] / 2) & (np.abs(by) <= b[4] / 2))
    area_a, area_b = a[3] * a[4], b[3] * b[4]
    inter, se_inter = p * area_a, np.sqrt(p * (1 - p) / n_samples) * area_a
    iou = inter / (area_a + area_b - inter)
    d_iou = (area_a + area_b) / (area_a + area_b - inter) ** 2            # d iou / d inter
    return iou, se_inter * d_iou


def fixture_pairs(n=20000, seed=5):
    """(a, b, n_designed): designed cases with known answers or hard geometry, then n random pairs (centres within
    +-50 m, b's centre a normal fraction of a's size away, heading noise 0.5 rad, size noise +-30 %), drawn from
    synth's counter-based streams and rounded to float32 (the reference's fp32 code sees those values); float64 arrays"""
    synth = importlib.import_module("3dal_pytorch_amd.synth")
    pi = np.pi
    rows = [
        ([0, 0, 0, 4, 2, 1.5, 0.3], [0, 0, 0, 4, 2, 1.5, 0.3]),              # identical -> 1
        ([0, 0, 0, 4, 2, 1, 0], [0, 0, 0, 2, 1, 1, 0]),                      # nested -> 0.25
        ([0, 0, 0, 2, 2, 1, 0], [1, 0, 0, 2, 2, 1, 0]),                      # half-shifted -> 1/3
        ([0, 0, 0, 2, 2, 1, 0], [2, 0, 0, 2, 2, 1, 0]),                      # edge-touching -> 0
        ([0, 0, 0, 2, 2, 1, 0], [0, 0, 0, 2, 2, 1, pi / 2]),                 # square vs itself at 90 deg -> 1
        ([0, 0, 0, 4, 1, 1, 0], [0, 0, 0, 4, 1, 1, pi / 2]),                 # cross -> 1/7
        ([3, -2, 0, 4.8, 1.8, 1.5, 0.7], [3, -2, 0, 4.8, 1.8, 1.5, 0.7 + pi]),   # yaw + pi -> 1
        ([5000.3, -3000.7, 1, 4.8, 1.8, 1.5, 0.2], [5000.3, -3000.7, 1, 4.8, 1.8, 1.5, 0.2]),  # identical, far out
        ([0, 0, 0, 10, 0.2, 1, 0.0], [0.5, 0.05, 0, 10, 0.2, 1, 0.01]),     # thin, nearly parallel
        ([0, 0, 0, 4, 2, 1, 0.25], [0.3, 0.2, 0.4, 4, 2, 1, 0.25]),          # equal yaws, offset in z too
        ([0, 0, 0, 4, 2, 1, 0], [10, 10, 0, 4, 2, 1, 1.0]),                  # far apart -> 0
    ]
    da, db = np.array([r[0] for r in rows], float), np.array([r[1] for r in rows], float)
    U, N = synth.uniform, synth.normal
    mean = np.array(synth.arch.MEAN_SIZE)[np.minimum((U(seed, "iou_cls", (n,)) * 3).astype(np.int64), 2)]
    a = np.concatenate([U(seed, "iou_axy", (n, 2), -50, 50), U(seed, "iou_az", (n, 1), -1, 1),
                        mean * U(seed, "iou_as", (n, 3), 0.7, 1.3), U(seed, "iou_ay", (n, 1), -pi, pi)], 1)
    b = np.concatenate([a[:, :2] + N(seed, "iou_bxy", (n, 2)) * a[:, 3:5] * 0.5, a[:, 2:3] + N(seed, "iou_bz", (n, 1), 0, 0.3),
                        a[:, 3:6] * U(seed, "iou_bs", (n, 3), 0.7, 1.3), a[:, 6:7] + N(seed, "iou_by", (n, 1), 0, 0.5)], 1)
    a, b = np.concatenate([da, a]), np.concatenate([db, b])
    return a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64), len(rows)
