"""Known answers of the voxel-fusion model (tests/np_fuse_model.py), computed by hand from the rule in include/slr.h.  No GPU."""
import numpy as np

import np_fuse_model as M


def _cloud(points, colors=None):
    """points: list of (x, y, z) or None (no point) -> one frame of H = 1 row"""
    W = len(points)
    xyz = np.zeros((1, 1, W, 3), np.float32)
    has = np.zeros((1, 1, W), np.uint8)
    for j, p in enumerate(points):
        if p is not None:
            xyz[0, 0, j] = p
            has[0, 0, j] = 1
    col = None if colors is None else np.asarray(colors, np.uint8).reshape(1, 1, W)
    return xyz, has, col


def test_negative_coordinates_take_the_floor():
    xyz, has, _ = _cloud([(-0.25, 0.0, 0.0)])
    out, cnt, _, rej = M.fuse(xyz, has, 1.0)
    # g = -0.25 -> v = -1, q = 0.75 * 2^24 = 12582912; centroid -1 + 12582912 / 2^24 = -0.25
    assert rej == 0 and cnt.tolist() == [1]
    assert out.tolist() == [[-0.25, 0.0, 0.0]]
    ok, key, q = M.keys_of(xyz.reshape(-1, 3), 1.0, (0, 0, 0))
    assert q[0].tolist() == [12582912, 0, 0]
    assert int(key[0]) == ((-1 + 2 ** 20) | (2 ** 20 << 21) | (2 ** 20 << 42))


def test_a_point_on_a_boundary_belongs_to_the_upper_cell():
    xyz, has, _ = _cloud([(1.0, 0.0, 0.0), (0.75, 0.0, 0.0)])
    out, cnt, _, _ = M.fuse(xyz, has, 0.5)
    # 1.0 / 0.5 = 2 exactly -> cell 2, q = 0; 0.75 / 0.5 = 1.5 -> cell 1, q = 2^23: two cells, in order of first occurrence
    assert cnt.tolist() == [1, 1]
    assert out.tolist() == [[1.0, 0.0, 0.0], [0.75, 0.0, 0.0]]


def test_the_remainder_term_of_the_centroid():
    xyz, has, _ = _cloud([(0.5, 0, 0), (0.25, 0, 0), (0.25, 0, 0)])
    out, cnt, _, _ = M.fuse(xyz, has, 1.0)
    # q = 2^23, 2^22, 2^22 -> S = 2^24, c = 3: S / c = 5592405, S % c = 1 -> (5592405 + 1/3) / 2^24 = 1/3 exactly in the
    # f64 evaluation order of the header: float32(1/3) -- the truncated quotient alone would give 5592405 / 2^24
    assert cnt.tolist() == [3]
    expect = np.float32((5592405.0 + 1.0 / 3.0) / 2 ** 24)
    assert out[0, 0] == expect and expect == np.float32(1.0 / 3.0)
    assert out[0, 0] != np.float32(5592405.0 / 2 ** 24)


def test_min_points_drops_sparse_cells_and_keeps_the_order():
    pts = [(5.5, 0, 0), (0.5, 0, 0), (0.6, 0, 0), (5.2, 0, 0), (9.0, 0, 0)]
    xyz, has, _ = _cloud(pts)
    out, cnt, _, _ = M.fuse(xyz, has, 1.0, min_points=2)
    assert cnt.tolist() == [2, 2]                      # cell 5 first (point 0), then cell 0 (point 1); cell 9 has one member
    # 5.2f = 5 + 3355440 / 2^24 and 0.6f = 10066330 / 2^24 exactly: S = 2^23 + 3355440 = 2 * 5872024, 2^23 + 10066330 = 2 * 9227469
    assert out[:, 0].tolist() == [np.float32(5 + 5872024 / 2 ** 24), np.float32(9227469 / 2 ** 24)]
    out1, cnt1, _, _ = M.fuse(xyz, has, 1.0, min_points=1)
    assert cnt1.tolist() == [2, 2, 1] and out1[2].tolist() == [9.0, 0.0, 0.0]


def test_non_finite_and_out_of_range_points_are_rejected():
    big = float(2 ** 20)
    pts = [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (big, 0, 0), (-big, 0, 0), (0, 0, big - 0.5), (1.5, 2.5, 3.5), None]
    xyz, has, _ = _cloud(pts)
    out, cnt, _, rej = M.fuse(xyz, has, 1.0)
    # NaN, +inf, -inf and the cell index 2^20 are rejected; -2^20 and 2^20 - 1 are the ends of the range; None is no point
    assert rej == 4
    assert cnt.tolist() == [1, 1, 1]
    assert out.tolist() == [[-big, 0.0, 0.0], [0.0, 0.0, big - 0.5], [1.5, 2.5, 3.5]]


def test_colour_is_rounded_to_nearest():
    xyz, has, col = _cloud([(0.1, 0, 0), (0.2, 0, 0), (3.1, 0, 0), (3.2, 0, 0), (3.3, 0, 0)], [10, 11, 10, 10, 11])
    _, cnt, oc, _ = M.fuse(xyz, has, 1.0, color=col)
    assert cnt.tolist() == [2, 3]
    assert oc.tolist() == [(21 + 1) // 2, (31 + 1) // 3] == [11, 10]


def test_transform_and_origin():
    xyz = np.zeros((2, 1, 1, 3), np.float32)
    xyz[0, 0, 0] = (0.25, 0, 0)
    xyz[1, 0, 0] = (0.25, 0, 0)
    has = np.ones((2, 1, 1), np.uint8)
    T = np.zeros((2, 3, 4), np.float32)
    T[:, :, :3] = np.eye(3)
    T[1, 0, 3] = 1.0                                   # frame 1 moves by +1 in x
    out, cnt, _, _ = M.fuse(xyz, has, 1.0, T=T)
    assert cnt.tolist() == [1, 1] and out[:, 0].tolist() == [0.25, 1.25]
    out, cnt, _, _ = M.fuse(xyz, has, 1.0, origin=(0.5, 0, 0), T=T)   # cells [-0.5, 0.5) and [0.5, 1.5)
    assert cnt.tolist() == [1, 1] and out[:, 0].tolist() == [0.25, 1.25]
    out, cnt, _, _ = M.fuse(xyz, has, 2.0, origin=(0.5, 0, 0), T=T)   # cell [-1.5, 0.5) and [0.5, 2.5)
    assert cnt.tolist() == [1, 1]
    out, cnt, _, _ = M.fuse(xyz, has, 4.0, origin=(-1.0, 0, 0), T=T)  # one cell [-1, 3): centroid 0.75
    assert cnt.tolist() == [2] and out[0].tolist() == [0.75, 0.0, 0.0]


def test_closed_form_of_a_constant_cloud():
    xyz = np.broadcast_to(np.float32([0.3, -1.7, 2.2]), (1, 7, 11, 3)).copy()
    has = np.ones((1, 7, 11), np.uint8)
    out, cnt, _, _ = M.fuse(xyz, has, 0.5, origin=(0.1, 0.2, 0.3))
    assert cnt.tolist() == [77]
    assert out[0].tolist() == M.fuse_constant((0.3, -1.7, 2.2), 77, 0.5, (0.1, 0.2, 0.3)).tolist()
