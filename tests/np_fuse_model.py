"""NumPy model of slr_fuse_voxels (include/slr.h), written out literally so that the GPU result can be compared bit for bit.

Keys: the three cell indices packed into 63 bits ((v_a + 2^20) << 21 a).  Cells: a stable argsort of the keys (what
np.unique(..., return_index=True, return_inverse=True) does inside), so each cell's first member is the smallest point index
(= `first`); sums: np.add.reduceat over the sorted u64 columns (exact; bincount weights are f64, np.add.at is too slow at 1e8
points).  The centroid is the f64 expression of the header, operation by operation."""
import numpy as np

Q = 2.0 ** 24
RANGE = 2.0 ** 20


def apply_T(T, X):
    """matCoordTrans (3x4 f32) * [X;1] with f64 accumulation in the order T0 x, T1 y, T2 z, T3 and one narrowing (apply_T of
    csrc/slr_device.hpp): X [m][3] f32 -> [m][3] f32"""
    T = np.asarray(T, np.float32).reshape(3, 4).astype(np.float64)
    Xd = X.astype(np.float64)
    out = np.empty_like(X, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):     # non-finite points stay non-finite (and are rejected)
        for r in range(3):
            s = T[r, 0] * Xd[:, 0]
            s = s + T[r, 1] * Xd[:, 1]
            s = s + T[r, 2] * Xd[:, 2]
            s = s + T[r, 3] * 1.0
            out[:, r] = s.astype(np.float32)
    return out


def keys_of(X, voxel, origin):
    """X [m][3] f32 (finite) -> (ok [m], key [m] u64, q [m][3] u64) -- ok False: a cell index outside [-2^20, 2^20)"""
    m = X.shape[0]
    ok = np.ones(m, bool)
    key = np.zeros(m, np.uint64)
    q = np.zeros((m, 3), np.uint64)
    for a in range(3):
        g = (X[:, a].astype(np.float64) - float(origin[a])) / float(voxel)
        v = np.floor(g)
        ok &= (v >= -RANGE) & (v < RANGE)
        vv = np.where(ok, v, 0.0)
        q[:, a] = np.where(ok, (g - vv) * Q, 0.0).astype(np.uint32)
        key |= (vv.astype(np.int64) + (1 << 20)).astype(np.uint64) << np.uint64(21 * a)
    return ok, key, q


def fuse(xyz, has, voxel, origin=(0.0, 0.0, 0.0), min_points=1, T=None, color=None):
    """-> (out_xyz [M][3] f32, count [M] u32, out_color [M] u8 or None, n_rejected)"""
    xyz = np.asarray(xyz, np.float32)
    has = np.asarray(has)
    n = 1 if has.ndim == 2 else has.shape[0]
    px = has.shape[-1] * has.shape[-2]
    X = xyz.reshape(-1, 3)
    e = np.flatnonzero(has.reshape(-1) != 0)
    P = X[e]
    if T is not None:
        T = np.asarray(T, np.float32).reshape(n, 12)
        f = e // px
        P = P.copy()
        for fr in np.unique(f):
            sel = f == fr
            P[sel] = apply_T(T[fr], P[sel])
    fin = np.isfinite(P).all(axis=1)
    ok, key, q = keys_of(np.where(fin[:, None], P, 0).astype(np.float32), voxel, origin)
    ok &= fin
    n_rejected = int((~ok).sum())
    e, key, q = e[ok], key[ok], q[ok]
    col = None if color is None else np.asarray(color).reshape(-1)[e].astype(np.uint64)
    if e.size == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), (None if color is None else np.zeros(0, np.uint8)), n_rejected
    order = np.argsort(key, kind="stable")
    ks = key[order]
    starts = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
    cnt = np.diff(np.append(starts, ks.size)).astype(np.uint64)
    first = e[order[starts]]
    S = np.stack([np.add.reduceat(q[order, a], starts) for a in range(3)], axis=1).astype(np.uint64)
    csum = np.add.reduceat(col[order], starts).astype(np.uint64) if col is not None else None
    keep = np.flatnonzero(cnt >= min_points)
    keep = keep[np.argsort(first[keep], kind="stable")]
    cnt, S, kk = cnt[keep], S[keep], ks[starts][keep]
    out = np.empty((keep.size, 3), np.float32)
    c = cnt.astype(np.float64)
    for a in range(3):
        v = ((kk >> np.uint64(21 * a)) & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20)
        frac = ((S[:, a] // cnt).astype(np.float64) + (S[:, a] % cnt).astype(np.float64) / c) / Q
        out[:, a] = (float(origin[a]) + (v.astype(np.float64) + frac) * float(voxel)).astype(np.float32)
    oc = None if csum is None else ((csum[keep] + cnt // np.uint64(2)) // cnt).astype(np.uint8)
    return out, cnt.astype(np.uint32), oc, n_rejected


def fuse_constant(value, count, voxel, origin=(0.0, 0.0, 0.0)):
    """closed form for `count` copies of one point (all in one cell): S_a = count q_a in Python integers"""
    P = np.asarray(value, np.float32).reshape(1, 3)
    ok, key, q = keys_of(P, voxel, origin)
    assert ok[0]
    out = np.empty(3, np.float32)
    for a in range(3):
        v = int((int(key[0]) >> (21 * a)) & 0x1FFFFF) - (1 << 20)
        S = int(q[0, a]) * count
        frac = (float(S // count) + float(S % count) / float(count)) / Q
        out[a] = np.float32(float(origin[a]) + (float(v) + frac) * float(voxel))
    return out
