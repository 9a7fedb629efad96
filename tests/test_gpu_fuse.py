"""slr_fuse_voxels on the MI355X against the NumPy model (tests/np_fuse_model.py), bit for bit: random clouds with long probe
chains, one cell holding 6e8 points, the bench's 8-frame verged batch with per-frame transforms, colour from the GE batch, both
memory kinds, determinism, the capacity contract and argument checks.  Output and scratch poisoning are on (tests/conftest.py)."""
import ctypes as C
import signal

import numpy as np
import pytest
import torch

import np_fuse_model as M
from util import bits_equal, np_of

pytestmark = pytest.mark.gpu

# Time limits per test, sized to each case on an MI355X (the bench-sized cases build and model 98 M points on the host).  SIGALRM
# ends a test between Python statements only: it cannot interrupt a call blocked inside the library.  What keeps a kernel from
# hanging is that every probe loop of kernels_fuse.hip is bounded; a run of the suite is wrapped in an outer time limit as well.
LIMITS_S = {"test_random_clouds_match_the_model": 60, "test_growing_capacity_with_millions_of_cells": 120,
            "test_one_cell_for_six_hundred_million_points": 180, "test_verged_batch_with_transforms": 300,
            "test_transform_equals_pretransformed_clouds": 240, "test_colour_from_the_ge_batch": 60,
            "test_memory_kinds_and_determinism": 60, "test_capacity_contract": 60, "test_invalid_arguments_are_refused_before_any_work": 30}


@pytest.fixture(autouse=True)
def _time_limit(request):
    limit = LIMITS_S[request.node.originalname]

    def expire(*_):
        raise TimeoutError("test exceeded %d s" % limit)
    old = signal.signal(signal.SIGALRM, expire)
    signal.alarm(limit)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _same(got, exp):
    gx, gc, gcol, grej = got
    ex, ec, ecol, erej = exp
    assert grej == erej, (grej, erej)
    assert bits_equal(np_of(gx), ex)
    assert np.array_equal(np_of(gc).astype(np.uint32), ec)
    if ecol is None:
        assert gcol is None
    else:
        assert bits_equal(np_of(gcol), ecol)


def _rotation(f):
    a, b = 0.03 * f, -0.02 * f
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.zeros((3, 4))
    T[:, :3] = Ry @ Rx
    T[:, 3] = (3.0 * f, -2.0 * f, 1.5 * f)
    return T.astype(np.float32)


def _random_cloud(rng, n, H, W, kind):
    if kind == "uniform":                                # nearly every point in a cell of its own: long probe chains
        xyz = rng.uniform(-50, 50, (n, H, W, 3)).astype(np.float32)
    else:                                                # a smooth surface per frame: runs of equal cells along the rows
        i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        xyz = np.empty((n, H, W, 3), np.float32)
        for f in range(n):
            xyz[f, ..., 0] = (j - W / 2) * 0.21 + f
            xyz[f, ..., 1] = (i - H / 2) * 0.19 - f
            xyz[f, ..., 2] = 400 + 20 * np.sin(i / 37.0 + f) * np.cos(j / 53.0) + rng.normal(0, 0.05, (H, W))
    has = (rng.random((n, H, W)) < 0.8).astype(np.uint8) * rng.integers(1, 256, (n, H, W), dtype=np.uint8)   # any non-zero byte
    bad = rng.random((n, H, W)) < 0.01
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 1e30]), int(bad.sum()))
    col = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    return xyz, has, col


@pytest.mark.parametrize("shape,kind,voxel", [((1, 64, 64), "uniform", 0.37), ((3, 100, 257), "uniform", 0.05),
                                              ((5, 480, 640), "surface", 0.5), ((2, 600, 800), "surface", 2.0)])
def test_random_clouds_match_the_model(ctx, shape, kind, voxel):
    rng = np.random.default_rng(sum(shape) + int(voxel * 100))
    n, H, W = shape
    xyz, has, col = _random_cloud(rng, n, H, W, kind)
    T = np.stack([_rotation(f) for f in range(n)])
    org = (-3.25, 1.5, 390.0)
    for mp in (1, 3):
        exp = M.fuse(xyz, has, voxel, org, mp, T=T, color=col)
        got = ctx.fuse_voxels(torch.from_numpy(xyz).cuda(), torch.from_numpy(has).cuda(), voxel, origin=org, min_points=mp, T=T,
                              color=torch.from_numpy(col).cuda())
        _same(got, exp)
        st = ctx.fuse_last_stats()
        assert st["points"] == n * H * W and st["distinct"] >= len(exp[1])
    # without colour, without T
    _same(ctx.fuse_voxels(xyz, has, voxel, origin=org), M.fuse(xyz, has, voxel, org))


def test_growing_capacity_with_millions_of_cells(ctx):
    """3.1 M distinct cells: the default capacity (2^20) is exceeded and grown; the result is the model's"""
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-1000, 1000, (1, 1500, 2100, 3)).astype(np.float32)
    has = np.ones((1, 1500, 2100), np.uint8)
    exp = M.fuse(xyz, has, 1.0)
    assert len(exp[1]) > (1 << 21)
    _same(ctx.fuse_voxels(torch.from_numpy(xyz).cuda(), torch.from_numpy(has).cuda(), 1.0), exp)


def test_one_cell_for_six_hundred_million_points(ctx):
    """maximum contention: every point in one cell, c > 2^29 so that S_a passes 2^53; closed-form model"""
    n, H, W = 40, 3000, 5000
    N = n * H * W
    assert N > (1 << 29) and N < (1 << 32)
    p = (12.34, -56.78, 901.5)
    dev = torch.device("cuda", 0)
    xyz = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
    xyz[..., 0], xyz[..., 1], xyz[..., 2] = p
    has = torch.ones((n, H, W), dtype=torch.uint8, device=dev)
    col = torch.full((n, H, W), 201, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    out, cnt, oc, rej = ctx.fuse_voxels(xyz, has, 4.0, origin=(0.5, 0.25, -0.125), color=col, max_voxels=1)
    assert rej == 0 and int(cnt[0]) == N and len(cnt) == 1 and cnt.dtype == torch.int64
    q = M.keys_of(np.float32([p]), 4.0, (0.5, 0.25, -0.125))[2][0]
    assert max(int(v) for v in q) * N > 2 ** 53
    assert bits_equal(np_of(out)[0], M.fuse_constant(p, N, 4.0, (0.5, 0.25, -0.125)))
    assert int(oc[0]) == 201
    del xyz, has, col
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def verged_batch(slr, synth):
    """the bench's timed batch: 8 frames of 4096 x 3000 from the 0.2 rad verged rig through slr_reconstruct_mf_batch"""
    W, H, F = 4096, 3000, 8
    c = slr.Context(0)
    rig = synth.make_verged_rig(W, H, 0.2, -0.15)
    c.set_calibration(rig["calib"])
    synth.install_verged_maps(c, rig, W, H)
    dev = torch.device("cuda", 0)
    stack = torch.zeros((F, 2, 14, H, W), dtype=torch.uint8, device=dev)
    for f in range(F):
        stack[f] = synth.render_mf_stack(W, H, seed=1234 + f, noise=2, device=dev)
    torch.cuda.synchronize()
    xyz, has = c.reconstruct_mf_batch(stack, 40, True, W=W)
    c.synchronize()
    del stack
    torch.cuda.empty_cache()
    yield xyz, has
    c.close()


@pytest.mark.parametrize("voxel", [0.5, 2.0])
def test_verged_batch_with_transforms(ctx, verged_batch, voxel):
    xyz, has = verged_batch
    T = np.stack([_rotation(f) for f in range(xyz.shape[0])])
    got = ctx.fuse_voxels(xyz, has, voxel, T=T)
    exp = M.fuse(np_of(xyz), np_of(has), voxel, T=T)
    assert len(exp[1]) > 1000 and exp[1].sum() > 10 ** 7
    _same(got, exp)


def test_transform_equals_pretransformed_clouds(ctx, verged_batch):
    xyz, has = verged_batch
    xyz, has = xyz[:2], has[:2]
    T = np.stack([_rotation(f + 1) for f in range(2)])
    hx = np_of(xyz)
    pre = np.stack([M.apply_T(T[f], hx[f].reshape(-1, 3)).reshape(hx[f].shape) for f in range(2)])
    a = ctx.fuse_voxels(xyz, has, 1.0, T=T, min_points=2)
    b = ctx.fuse_voxels(torch.from_numpy(pre).cuda(), has, 1.0, min_points=2)
    _same(a, (np_of(b[0]), np_of(b[1]).astype(np.uint32), None, b[3]))


def test_colour_from_the_ge_batch(ctx, slr, synth):
    W, H = 1024, 768
    calib, _ = synth.make_calibration(W, H)
    ctx.set_calibration(calib)
    ncol = synth.gray_num_bits(W)
    dev = torch.device("cuda", 0)
    stack = torch.stack([synth.render_gray_stack(W, H, W, seed=400 + f, noise=2, device=dev) for f in range(2)]).contiguous()
    torch.cuda.synchronize()
    xyz, has, col = ctx.reconstruct_batch(slr.capi.MODE_GE, stack, 40, 3, n_col_bits=ncol, scan_w=W, rectify=False, have_color=True)
    ctx.synchronize()
    assert int(has.sum()) > 10000
    for voxel in (0.5, 3.0):
        got = ctx.fuse_voxels(xyz, has, voxel, color=col)
        _same(got, M.fuse(np_of(xyz), np_of(has), voxel, color=np_of(col)))
        assert len(np.unique(np_of(got[2]))) > 1 and (np_of(got[1]) > 1).any()


def test_memory_kinds_and_determinism(ctx):
    rng = np.random.default_rng(11)
    xyz, has, col = _random_cloud(rng, 3, 240, 320, "surface")
    T = np.stack([_rotation(f) for f in range(3)])
    host = ctx.fuse_voxels(xyz, has, 0.3, T=T, color=col, min_points=2)
    dx, dh, dc = (torch.from_numpy(a).cuda() for a in (xyz, has, col))
    d1 = ctx.fuse_voxels(dx, dh, 0.3, T=torch.from_numpy(T), color=dc, min_points=2)
    d2 = ctx.fuse_voxels(dx, dh, 0.3, T=T, color=dc, min_points=2)
    assert isinstance(host[0], np.ndarray) and d1[0].is_cuda
    _same(d1, (host[0], host[1], host[2], host[3]))
    _same(d2, (host[0], host[1], host[2], host[3]))
    # one frame given as [H][W][3]
    one = ctx.fuse_voxels(xyz[1], has[1], 0.3)
    _same(one, M.fuse(xyz[1], has[1], 0.3))


def _raw_call(ctx, slr, desc, xyz, has, out, cnt, color=None, out_color=None, T=None):
    nv, nrej = C.c_uint32(0xDEAD), C.c_uint64(0)
    p = lambda a: C.c_void_p(None) if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    st = ctx.lib.slr_fuse_voxels(ctx.h, C.byref(desc) if desc is not None else None, p(xyz), p(has), p(color), p(T), p(out), p(cnt),
                                 p(out_color), C.byref(nv), C.byref(nrej), C.c_int(slr.capi.MEM_HOST))
    return st, nv.value, nrej.value


def test_capacity_contract(ctx, slr):
    D = 5000
    xyz = np.zeros((1, 1, D, 3), np.float32)
    xyz[0, 0, :, 0] = np.arange(D, dtype=np.float32) * 2 + 0.5       # D distinct cells of edge 1
    has = np.ones((1, 1, D), np.uint8)
    with pytest.raises(slr.SlrError) as e:
        ctx.fuse_voxels(xyz, has, 1.0, max_voxels=D - 1)
    assert e.value.status == slr.capi.ERR_OOM and e.value.n_voxels == D and "max_voxels" in str(e.value)
    got = ctx.fuse_voxels(xyz, has, 1.0, max_voxels=D)
    _same(got, M.fuse(xyz, has, 1.0))
    # nothing is written on overflow, and nothing past n_voxels on success (host buffers with sentinels)
    cap = D + 100
    out = np.full((cap, 3), 7.0, np.float32)
    cnt = np.full(cap, 0xA5A5A5A5, np.uint32)
    desc = slr.capi.FuseDesc(1, D, 1, 1.0, (C.c_double * 3)(0, 0, 0), 1, D - 1)
    st, nv, nrej = _raw_call(ctx, slr, desc, xyz, has, out, cnt)
    assert st == slr.capi.ERR_OOM and nv > D - 1 and nrej == 0
    assert (out == 7.0).all() and (cnt == 0xA5A5A5A5).all()
    desc.max_voxels = cap
    st, nv, _ = _raw_call(ctx, slr, desc, xyz, has, out, cnt)
    assert st == slr.capi.OK and nv == D
    assert (out[D:] == 7.0).all() and (cnt[D:] == 0xA5A5A5A5).all() and (cnt[:D] == 1).all()
    # far more cells than the capacity: the insert gives up early and reports a count above it
    rng = np.random.default_rng(3)
    big = rng.uniform(-1e4, 1e4, (1, 1000, 1000, 3)).astype(np.float32)
    bh = np.ones((1, 1000, 1000), np.uint8)
    with pytest.raises(slr.SlrError) as e:
        ctx.fuse_voxels(big, bh, 1.0, max_voxels=1000)
    assert e.value.status == slr.capi.ERR_OOM and e.value.n_voxels > 1000
    # and the context is fine afterwards
    _same(ctx.fuse_voxels(xyz, has, 1.0), M.fuse(xyz, has, 1.0))


def test_invalid_arguments_are_refused_before_any_work(ctx, slr):
    xyz = np.zeros((1, 2, 2, 3), np.float32)
    has = np.ones((1, 2, 2), np.uint8)
    out, cnt = np.zeros((8, 3), np.float32), np.zeros(8, np.uint32)
    col, ocol = np.zeros((1, 2, 2), np.uint8), np.zeros(8, np.uint8)
    ctx.fuse_voxels(xyz, has, 1.0)
    before = ctx.fuse_last_stats()
    D = slr.capi.FuseDesc
    z = (C.c_double * 3)(0, 0, 0)
    bad = [D(1, 2, 2, 0.0, z, 1, 8), D(1, 2, 2, -1.0, z, 1, 8), D(1, 2, 2, float("nan"), z, 1, 8), D(1, 2, 2, float("inf"), z, 1, 8),
           D(1, 2, 2, 1.0, (C.c_double * 3)(0, float("nan"), 0), 1, 8), D(1, 2, 2, 1.0, (C.c_double * 3)(0, 0, float("-inf")), 1, 8),
           D(1, 2, 2, 1.0, z, 0, 8), D(1, 2, 2, 1.0, z, 1, 0), D(1, 2, 2, 1.0, z, 1, (1 << 30) + 1), D(0, 2, 2, 1.0, z, 1, 8),
           D(1, 0, 2, 1.0, z, 1, 8), D(1, 2, -1, 1.0, z, 1, 8), D(4096, 1024, 1024, 1.0, z, 1, 8)]
    for d in bad:
        st, _, _ = _raw_call(ctx, slr, d, xyz, has, out, cnt)
        assert st == slr.capi.ERR_INVALID_ARG, (d.n_frames, d.W, d.H, d.voxel, list(d.origin), d.min_points, d.max_voxels)
    good = D(1, 2, 2, 1.0, z, 1, 8)
    assert _raw_call(ctx, slr, good, xyz, has, out, cnt, color=col)[0] == slr.capi.ERR_INVALID_ARG          # colour without out_color
    assert _raw_call(ctx, slr, good, xyz, has, out, cnt, out_color=ocol)[0] == slr.capi.ERR_INVALID_ARG
    assert _raw_call(ctx, slr, good, None, has, out, cnt)[0] == slr.capi.ERR_INVALID_ARG
    assert _raw_call(ctx, slr, None, xyz, has, out, cnt)[0] == slr.capi.ERR_INVALID_ARG
    assert ctx.fuse_last_stats() == before                     # no refused call got as far as the kernels
    assert _raw_call(ctx, slr, good, xyz, has, out, cnt)[:2] == (slr.capi.OK, 1)
    with pytest.raises(ValueError):
        ctx.fuse_voxels(xyz, has, 1.0, T=np.eye(3, 4, dtype=np.float32).reshape(1, 12).repeat(2, 0))
