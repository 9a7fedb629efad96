"""Point-to-plane ICP on the MI355X (slr_cloud_normals, slr_icp_linearize, slr_register_icp) against the NumPy model
(tests/np_icp_model.py): normals bit for bit, a bench-sized linearisation with the model's exact inlier count, its sums to 1e-9 and
each within the rounding bound of the kernel's summation tree,
a known motion recovered, a verged-rig frame registered back onto itself, bit-identical results across calls and memory kinds,
stop reason 3, and argument checks.  Output and scratch poisoning are on (tests/conftest.py)."""
import ctypes as C
import signal

import numpy as np
import pytest
import torch

import np_icp_model as M
from util import bits_equal, np_of

pytestmark = pytest.mark.gpu

# Time limits per test, sized to each case on an MI355X (the bench-sized case renders and models 12 M points on the host, and sums
# 2 x 28 x 12 M terms exactly).  SIGALRM ends a test between Python statements only; every kernel of kernels_icp.hip is a bounded
# loop, and the suite runs under an outer time limit as well.
LIMITS_S = {"test_normals_match_the_model_bit_for_bit": 60, "test_linearize_at_bench_size_matches_the_model": 360,
            "test_register_recovers_a_known_motion": 120, "test_verged_frame_registers_onto_itself": 120,
            "test_bit_identical_across_calls_and_memory_kinds": 120, "test_too_few_inliers_stops_with_reason_3": 60,
            "test_invalid_arguments_are_refused_before_any_work": 30}


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


def _pinhole(W, H):
    return (1.0 * W, 1.0 * W, 0.5 * W + 0.3, 0.5 * H - 0.4)


def _errors(T, E):
    dR = np.asarray(T, np.float64)[:, :3] @ np.asarray(E, np.float64)[:, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    return ang, np.abs(np.asarray(T, np.float64)[:, 3] - np.asarray(E, np.float64)[:, 3]).max()


def _rough_grid(rng, H, W):
    """a smooth surface with holes, depth jumps, non-finite points and a few exactly repeated points"""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 900 + 40 * np.sin(i / 17.0) * np.cos(j / 23.0) + rng.normal(0, 0.2, (H, W))
    z[:, W // 3:] += 60.0                                    # a step well beyond max_edge
    xyz = np.stack([(j - W / 2) * z / W, (i - H / 2) * z / W, z], -1).astype(np.float32)
    has = ((rng.random((H, W)) < 0.9) * rng.integers(1, 256, (H, W))).astype(np.uint8)
    bad = rng.random((H, W)) < 0.01
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), int(bad.sum()))
    if W >= 8:
        xyz[H // 2, 5:8] = xyz[H // 2, 6]                    # m == 0 (a degenerate cross product)
    return xyz, has


@pytest.mark.parametrize("H,W,max_edge", [(1, 1, 1.0), (2, 7, 5.0), (3, 3, 50.0), (97, 131, 15.0), (480, 640, 8.0)])
def test_normals_match_the_model_bit_for_bit(ctx, H, W, max_edge):
    rng = np.random.default_rng(H * W)
    xyz, has = _rough_grid(rng, H, W)
    en, ev = M.normals(xyz, has, max_edge)
    gn, gv = ctx.cloud_normals(xyz, has, max_edge)
    assert bits_equal(gv, ev) and bits_equal(gn, en)
    dn, dv = ctx.cloud_normals(torch.from_numpy(xyz).cuda(), torch.from_numpy(has).cuda(), max_edge)
    ctx.synchronize()
    assert bits_equal(np_of(dv), ev) and bits_equal(np_of(dn), en)
    if H * W > 1000:
        assert 0.3 < ev.mean() < 0.9


@pytest.fixture(scope="module")
def bench_pair():
    """two 4096 x 3000 renders of the analytic scene, the second from a camera moved by the known motion"""
    W, H = 4096, 3000
    ph = _pinhole(W, H)
    A = M.motion()
    xa, ha = M.render(W, H, ph)
    xb, hb = M.render(W, H, ph, A)
    return ph, A, xa, ha, xb, hb


def test_linearize_at_bench_size_matches_the_model(ctx, bench_pair):
    ph, A, xa, ha, xb, hb = bench_pair
    nrm, nv = M.normals(xa, ha, 10.0)
    src_has = hb.copy()
    src_has[::7, ::5] = 0
    dx, dh = torch.from_numpy(xa).cuda(), torch.from_numpy(ha).cuda()
    sx, sh = torch.from_numpy(xb).cuda(), torch.from_numpy(src_has).cuda()
    for T, has in ((np.eye(3, 4), None), (M.invert(M.motion(deg=1.2, t=(1.5, -2.0, 1.0))), src_has)):
        es, en = M.linearize(xb, has, xa, ha, nrm, nv, ph, T, 30.0)
        gs, gn = ctx.icp_linearize(sx, sh if has is not None else None, dx, dh, ph, T, 30.0, 10.0)
        assert gn == en and en > 0.5 * xa.shape[0] * xa.shape[1], (gn, en)
        assert np.abs(gs - es).max() <= 1e-9 * np.abs(es).max(), np.abs(gs - es).max() / np.abs(es).max()
        # and each entry on its own, within the rounding bound of the kernel's summation tree around the exactly rounded sum
        terms, tn = M.linearize_terms(xb, has, xa, ha, nrm, nv, ph, T, 30.0)
        assert tn == en
        M.assert_within_rounding_bound(gs, terms, xb.shape[0] * xb.shape[1])
        del terms


def test_register_recovers_a_known_motion(ctx):
    W, H = 1024, 768
    ph = _pinhole(W, H)
    A = M.motion()
    xa, ha = M.render(W, H, ph)
    xb, hb = M.render(W, H, ph, A)
    T, res = ctx.register_icp(xb, hb, xa, ha, ph, max_dist=40.0)
    ang, dt = _errors(res["T64"], M.invert(A))
    assert res["stop_reason"] == 1 and res["iterations"] >= 2, res
    assert ang < 0.01 and dt < 0.01, (ang, dt)
    assert T.dtype == np.float32 and bits_equal(T, res["T64"].astype(np.float32))
    ET, eres = M.register(xb, hb, xa, ha, ph, max_dist=40.0)
    assert res["iterations"] == eres["iterations"] and res["inliers"] == eres["inliers"]
    assert np.abs(res["T64"] - ET).max() < 1e-7


def rectified_calib(slr, rig):
    """the rig's calibration with each camera as the rectified pinhole of its P (no distortion): K4 then triangulates every pixel
    on its own ray of the rectified left camera, the pinhole pinhole_from_Q(Q) describes.  (The reference undistorts the rectified
    pixels once more with the raw cameras' distortion; its clouds sit up to several pixels off these rays.)"""
    P1, P2 = rig["P1"], rig["P2"]
    cam = [slr.make_camera((P[0, 0], P[1, 1]), (P[0, 2], P[1, 2]), (0.0,) * 5) for P in (P1, P2)]
    return slr.make_calib(cam[0], cam[1], rig["Q"])


def test_verged_frame_registers_onto_itself(ctx, slr, synth):
    """a reconstructed verged-rig frame registered back onto itself.  K4 matches whole pixels, so the cloud is terraced, and the
    unweighted loop comes back only from close starts with tight bounds (profiles/icp_sweep_results.txt):
    from 0.03 deg / 0.3 mm and from a 0.5 mm shift, with 5 mm bounds.  From identity the step is exactly zero: every point lands on its
    own pixel (pinhole_from_Q is the grid K4 triangulated on)."""
    W, H = 2048, 1536
    c = slr.Context(0)
    rig = synth.make_verged_rig(W, H, 0.2, -0.15)
    c.set_calibration(rectified_calib(slr, rig))
    synth.install_verged_maps(c, rig, W, H)
    stack = synth.render_mf_stack(W, H, seed=1234, noise=2, device=torch.device("cuda", 0))[None].contiguous()
    torch.cuda.synchronize()
    xyz, has = c.reconstruct_mf_batch(stack, 40, True, W=W)
    c.synchronize()
    c.close()
    xyz, has = xyz[0].contiguous(), has[0].contiguous()
    assert int(has.sum()) > 0.3 * W * H
    ph = slr.pinhole_from_Q(rig["Q"])
    src, sh = xyz.view(-1, 3), has.view(-1)
    for P in (M.motion(axis=(-0.4, 0.9, 0.3), deg=0.03, t=(0.2, -0.2, 0.1)), M.motion(deg=0.0, t=(0.5, 0.0, 0.0))):
        s0, n0 = ctx.icp_linearize(src, sh, xyz, has, ph, P, 5.0, 5.0)
        T, res = ctx.register_icp(src, sh, xyz, has, ph, T_init=P.astype(np.float32), max_dist=5.0, max_edge=5.0)
        ang, dt = _errors(res["T64"], np.eye(3, 4))
        ang0, dt0 = _errors(P, np.eye(3, 4))
        assert res["stop_reason"] == slr.capi.ICP_CONVERGED and res["iterations"] > 1, res
        assert ang < 0.02 and (ang < 1e-3 if ang0 == 0 else ang < ang0), (ang, ang0)
        assert dt < 0.01 and dt < dt0 / 10, (dt, dt0)
        s1, n1 = ctx.icp_linearize(src, sh, xyz, has, ph, res["T64"], 5.0, 5.0)
        assert n1 > 2 * n0 and s1[27] / n1 < 0.5 * s0[27] / n0, (n0, n1)
    T, res = ctx.register_icp(src, sh, xyz, has, ph, max_dist=50.0, max_edge=50.0)
    _, nv = ctx.cloud_normals(xyz, has, 50.0)
    ctx.synchronize()
    assert res["stop_reason"] == slr.capi.ICP_CONVERGED and res["iterations"] == 1 and res["rms"] == 0.0, res
    n_normal = int(nv.sum())
    # (a few dozen points of the frame land a rounding off their pixel centre and take the neighbour's pixel)
    assert n_normal > 0.2 * W * H and abs(res["inliers"] - n_normal) <= 1e-3 * n_normal, (res["inliers"], n_normal)
    assert bits_equal(T, np.eye(3, 4, dtype=np.float32))


def test_bit_identical_across_calls_and_memory_kinds(ctx):
    W, H = 640, 480
    ph = _pinhole(W, H)
    xa, ha = M.render(W, H, ph)
    xb, hb = M.render(W, H, ph, M.motion())
    T0 = M.motion(deg=0.2, t=(0.5, 0.0, -0.5)).astype(np.float32)
    host = ctx.register_icp(xb, hb, xa, ha, ph, T_init=T0, max_dist=40.0)
    d = [torch.from_numpy(a).cuda() for a in (xb, hb, xa, ha)]
    for _ in range(2):
        dev = ctx.register_icp(*d, ph, T_init=torch.from_numpy(T0), max_dist=40.0)
        assert bits_equal(dev[0], host[0]) and bits_equal(dev[1]["T64"], host[1]["T64"])
        assert {k: v for k, v in dev[1].items() if k != "T64"} == {k: v for k, v in host[1].items() if k != "T64"}
    s1 = ctx.icp_linearize(xb, hb, xa, ha, ph, host[1]["T64"], 40.0, 10.0)
    s2 = ctx.icp_linearize(*d, ph, host[1]["T64"], 40.0, 10.0)
    assert bits_equal(s1[0], s2[0]) and s1[1] == s2[1] > 0


def test_too_few_inliers_stops_with_reason_3(ctx, slr):
    W, H = 320, 240
    ph = _pinhole(W, H)
    xa, ha = M.render(W, H, ph)
    T0 = np.float32([[1, 0, 0, 5000], [0, 1, 0, 0], [0, 0, 1, 0]])          # every point moved 5 m sideways: off the grid
    T, res = ctx.register_icp(xa, ha, xa, ha, ph, T_init=T0, max_dist=20.0)
    assert res["stop_reason"] == slr.capi.ICP_FEW_INLIERS and res["iterations"] == 0 and res["inliers"] < 6
    assert bits_equal(T, T0)
    # and a planar scene is singular
    scene = ([("plane", (0.0, 0.0, -1.0), -1000.0)], [])
    xp, hp = M.render(W, H, ph, scene=scene)
    T, res = ctx.register_icp(xp, hp, xp, hp, ph, max_dist=20.0)
    assert res["stop_reason"] == slr.capi.ICP_SINGULAR and res["iterations"] == 0 and res["inliers"] > 1000


def test_invalid_arguments_are_refused_before_any_work(ctx, slr):
    W, H = 16, 12
    xyz = np.ones((H, W, 3), np.float32)
    has = np.ones((H, W), np.uint8)
    Tout = np.full(12, 7.0, np.float32)
    sums = np.full(28, 7.0)
    p = lambda a: C.c_void_p(None) if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    D = slr.capi.IcpDesc

    def desc(**kw):
        f = dict(W=W, H=H, fx=20.0, fy=20.0, cx=8.0, cy=6.0, max_dist=5.0, max_edge=5.0, max_iters=10, stop_rot=1e-6, stop_trans=1e-4,
                 min_inliers=6)
        f.update(kw)
        return D(*[f[k] for k, _ in D._fields_])

    def reg(d, src=xyz, dst=xyz, dh=has, out=Tout, mem=slr.capi.MEM_HOST):
        res = slr.capi.IcpResult()
        res.iterations = -7
        st = ctx.lib.slr_register_icp(ctx.h, C.byref(d) if d is not None else None, p(src), None, C.c_size_t(W * H), p(dst), p(dh),
                                      None, p(out), C.byref(res), C.c_int(mem))
        return st, res.iterations

    def lin(d, T=np.eye(3, 4).reshape(12)):
        n = C.c_uint64(0)
        return ctx.lib.slr_icp_linearize(ctx.h, C.byref(d), p(xyz), None, C.c_size_t(W * H), p(xyz), p(has), p(T), p(sums),
                                         C.byref(n), C.c_int(slr.capi.MEM_HOST))

    nan, inf = float("nan"), float("inf")
    bad = [desc(W=0), desc(H=-1), desc(W=1 << 16, H=1 << 15), desc(fx=0.0), desc(fy=-1.0), desc(fx=nan), desc(cx=inf), desc(cy=nan),
           desc(max_dist=0.0), desc(max_dist=nan), desc(max_edge=-1.0), desc(max_edge=inf), desc(max_iters=0), desc(max_iters=101),
           desc(stop_rot=-1.0), desc(stop_trans=nan), desc(min_inliers=5)]
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        for d in bad:
            assert reg(d) == (slr.capi.ERR_INVALID_ARG, -7), [getattr(d, k) for k, _ in D._fields_]
            assert lin(d) == slr.capi.ERR_INVALID_ARG
        good = desc()
        assert reg(None)[0] == slr.capi.ERR_INVALID_ARG
        assert reg(good, src=None)[0] == reg(good, dst=None)[0] == reg(good, dh=None)[0] == reg(good, out=None)[0] == slr.capi.ERR_INVALID_ARG
        assert reg(good, mem=7)[0] == slr.capi.ERR_INVALID_ARG
        assert lin(good, T=np.array([1, 0, 0, nan, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)) == slr.capi.ERR_INVALID_ARG
        nrm, nv = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.uint8)
        for args in ((W, H, 0.0), (W, H, nan), (0, H, 1.0), (W, 0, 1.0)):
            assert ctx.lib.slr_cloud_normals(ctx.h, p(xyz), p(has), C.c_int(args[0]), C.c_int(args[1]), C.c_double(args[2]), p(nrm), p(nv),
                                             C.c_int(slr.capi.MEM_HOST)) == slr.capi.ERR_INVALID_ARG
        assert (Tout == 7.0).all() and (sums == 7.0).all()
        assert not any(k.startswith("slr_icp_") for k in ctx.profile())      # no refused call got as far as a kernel
        assert reg(good) == (slr.capi.OK, 0)                                  # one repeated point: no normals, so stop reason 3 at once
        assert "slr_icp_normals" in ctx.profile()
    finally:
        ctx.profile_enable(False)
    with pytest.raises(ValueError):
        ctx.register_icp(xyz, has[:-1], xyz, has, (20.0, 20.0, 8.0, 6.0))
    with pytest.raises(ValueError):
        ctx.register_icp(xyz, has, xyz, has, (20.0, 20.0, 8.0, 6.0), T_init=np.eye(3))
