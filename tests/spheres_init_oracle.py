"""Numpy statement of the sphere initialisation (tssplat_amd/spheres_init.py, DESIGN.md "Sphere initialisation"): visual hull, exact
squared Euclidean distance transform, greedy ball cover.  numpy only (scipy may be absent where the GPU tests run).

The device results must equal these bit for bit, so every decision is an integer comparison, a float32 operation that numpy rounds
on its own (a multiply and an add are never fused here), or one float64 product of exactly representable integers.

Grid: G voxels per axis over [lo, hi]^3, h = (hi - lo) / G in float64, voxel (i, j, k) has the flat index (i G + j) G + k (C order)
and the centre float32(lo + (index + 0.5) h) per axis."""
import numpy as np

SENTINEL = 1 << 30      # a line without a false voxel: loses every min; + 511^2 stays below 2^31
MAX_GRID = 512


def voxel_centres(grid, bounds=(-1.0, 1.0)):
    """float32 [G]: the voxel centres along one axis."""
    lo, hi = float(bounds[0]), float(bounds[1])
    h = (hi - lo) / grid
    return (lo + (np.arange(grid, dtype=np.float64) + 0.5) * h).astype(np.float32)


def visual_hull(alpha, mvp, grid=72, bounds=(-1.0, 1.0), threshold=0.5, channel=0):
    """bool [G, G, G]: the voxels whose centre every view sees on the object.  alpha float32 [B, H, W, C], mvp float32 [B, 4, 4]."""
    alpha = np.asarray(alpha, dtype=np.float32)
    mvp = np.asarray(mvp, dtype=np.float32)
    B, H, W = alpha.shape[:3]
    c = voxel_centres(grid, bounds)
    X, Y, Z = (a.reshape(-1) for a in np.meshgrid(c, c, c, indexing="ij"))
    one, half, thr = np.float32(1.0), np.float32(0.5), np.float32(threshold)
    inside = np.ones(X.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            m = mvp[b]
            c0, c1, c3 = (((m[r, 0] * X + m[r, 1] * Y) + m[r, 2] * Z) + m[r, 3] for r in (0, 1, 3))
            assert c0.dtype == np.float32
            ok = c3 > 0                                       # (NaN > 0 is false)
            safe = np.where(ok, c3, one)
            nx, ny = c0 / safe, c1 / safe                     # IEEE float32 division
            ok &= (np.abs(nx) < one) & (np.abs(ny) < one)
            fx = np.floor(((nx + one) * half) * np.float32(W))
            fy = np.floor(((ny + one) * half) * np.float32(H))
            px = np.minimum(W - 1, np.where(ok, fx, 0).astype(np.int64))
            py = np.minimum(H - 1, np.where(ok, fy, 0).astype(np.int64))
            assert px.min() >= 0 and py.min() >= 0            # |ndc| < 1 alone keeps the index at or above 0
            occ = alpha[b, :, :, channel] > thr               # strict; NaN > thr is false
            inside &= ok & occ[py, px]
    return inside.reshape(grid, grid, grid)


def distance_transform_sq(mask):
    """int32 [G, G, G]: exact squared distance (voxel units) to the nearest false voxel, 0 where the mask is false; nothing outside
    the array is background (scipy.ndimage.distance_transform_edt(mask) ** 2).  A mask without a false voxel: ValueError."""
    mask = np.asarray(mask, dtype=bool)
    if mask.all():
        raise ValueError("distance_transform_sq: the mask has no false voxel")
    f = np.where(mask, np.int64(SENTINEL), np.int64(0))
    G = mask.shape[0]
    idx = np.arange(G, dtype=np.int64)
    for axis in (2, 1, 0):
        f = np.moveaxis(f, axis, -1)
        out = np.full_like(f, np.iinfo(np.int64).max)
        for j in range(G):                                   # out[..., a] = min_j f[..., j] + (a - j)^2
            np.minimum(out, f[..., j:j + 1] + (idx - j) ** 2, out=out)
        f = np.moveaxis(out, -1, axis)
    assert f.max() < SENTINEL
    return np.ascontiguousarray(f).astype(np.int32)


def cover_constants(grid, bounds, min_radius, shrink):
    """(h, s2, hs2, m2) as the host computes them once, in float64."""
    h = (float(bounds[1]) - float(bounds[0])) / grid
    s, m = float(shrink), float(min_radius)
    return h, s * s, (h * s) * (h * s), m * m


def greedy_cover(hull, d2, n_spheres, bounds=(-1.0, 1.0), min_radius=0.05, shrink=0.92):
    """(flat int64 [S], q int32 [S], uncovered bool [G, G, G]): the largest uncovered inscribed ball, repeated."""
    hull = np.asarray(hull, dtype=bool)
    G = hull.shape[0]
    _, s2, hs2, m2 = cover_constants(G, bounds, min_radius, shrink)
    I, J, K = np.meshgrid(*(np.arange(G, dtype=np.int64),) * 3, indexing="ij")
    uncovered = hull.copy()
    flat, qs = [], []
    for _ in range(int(n_spheres)):
        score = np.where(uncovered, np.asarray(d2, dtype=np.int64), -1).reshape(-1)
        k = int(np.argmax(score))                            # the first maximum: the lowest flat index among equals
        q = int(score[k])
        if q <= 0 or float(q) * hs2 < m2:                    # nothing uncovered (-1), q == 0, or a radius below min_radius
            break
        flat.append(k)
        qs.append(q)
        i, j, kk = np.unravel_index(k, hull.shape)
        D2 = (I - i) ** 2 + (J - j) ** 2 + (K - kk) ** 2
        uncovered &= ~(D2.astype(np.float64) <= float(q) * s2)
    return np.asarray(flat, dtype=np.int64), np.asarray(qs, dtype=np.int32), uncovered


def centres_and_radii(flat, q, grid, bounds=(-1.0, 1.0), shrink=0.92):
    """(pt float32 [S, 3], r float32 [S]) of the records of greedy_cover."""
    c = voxel_centres(grid, bounds)
    h = (float(bounds[1]) - float(bounds[0])) / grid
    flat = np.asarray(flat, dtype=np.int64)
    ijk = np.stack(np.unravel_index(flat, (grid, grid, grid)), axis=1).reshape(-1, 3)
    r = (np.sqrt(np.asarray(q, dtype=np.float64)) * h * float(shrink)).astype(np.float32)
    return c[ijk].astype(np.float32).reshape(-1, 3), r.reshape(-1)


def init_spheres(alpha, mvp, n_spheres, grid=72, bounds=(-1.0, 1.0), threshold=0.5, channel=0, min_radius=0.05, shrink=0.92):
    """dict(pt, r, flat, q, hull, uncovered, hull_fraction, uncovered_fraction): the three stages in a row.  A hull that fills the
    whole cube has no distance transform: ValueError, as from distance_transform_sq."""
    hull = visual_hull(alpha, mvp, grid, bounds, threshold, channel)
    d2 = distance_transform_sq(hull)
    flat, q, uncovered = greedy_cover(hull, d2, n_spheres, bounds, min_radius, shrink)
    pt, r = centres_and_radii(flat, q, grid, bounds, shrink)
    n_hull = int(hull.sum())
    return {"pt": pt, "r": r, "flat": flat, "q": q, "hull": hull, "uncovered": uncovered, "hull_fraction": n_hull / float(grid ** 3),
            "uncovered_fraction": int(uncovered.sum()) / float(max(1, n_hull))}
