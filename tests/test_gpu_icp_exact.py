"""Point-to-plane ICP on the MI355X held to exact references (tests/np_icp_model.py): sums bit for bit against a closed form on a
fixture where f64 summation is exact in any order, over n_src at the edges of the kernel's summation tree, in any source order and
on both memory kinds; every sum within the rounding bound of that tree against an exactly rounded reference on general geometry with
an anisotropic pinhole; the half-pixel rounding, the gate at equality and the rejection of degenerate points; one step of the loop bit
for bit against the host's solve and update; stop reasons 2, 3 and 4 at their edges; an empty source.  Output and scratch poisoning
are on (tests/conftest.py)."""
import ctypes as C
import math
import signal

import numpy as np
import pytest
import torch

import np_icp_model as M
from util import bits_equal

pytestmark = pytest.mark.gpu

# Time limits per test, sized to each case on an MI355X (the rounding-bound test sums 28 x 0.8 M terms exactly on the host).  SIGALRM
# ends a test between Python statements only; every kernel of kernels_icp.hip is a bounded loop, and the suite runs under an outer
# time limit as well.
LIMITS_S = {"test_wall_sums_are_exact_at_every_size_order_and_memory_kind": 60,
            "test_wall_sums_are_exact_with_inliers_planted_at_the_tree_edges": 60,
            "test_sums_are_within_the_rounding_bound_on_an_anisotropic_scene": 180,
            "test_half_pixels_round_up_on_u_and_v": 30, "test_gate_keeps_equality": 30,
            "test_degenerate_points_are_rejected": 30, "test_one_step_is_the_host_solve_and_update_bit_for_bit": 60,
            "test_max_iters_stops_with_reason_2": 60, "test_min_inliers_at_its_boundary": 30,
            "test_singular_beyond_the_plane": 60, "test_empty_source": 30}

U = 2.0 ** -53                     # unit roundoff of f64
SWEEP = [1, 63, 64, 65, 1023, 1024, 1025, 262143, 262144, 262145, 5 * 262144 + 777]
WW, WH = 1024, 768                 # the wall fixture's grid (<= 2048 wide: every wall point lands on its own pixel)


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


def _anisotropic(W, H):
    return (1.0 * W, 1.1 * W, 0.5 * W + 0.3, 0.5 * H - 0.4)


def _dev(*arrs):
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrs]      # a copy: no negative strides


def _lin(ctx, src, sh, dst, dh, ph, T, max_dist, device=False, max_edge=10.0):
    if device:
        src, sh, dst, dh = _dev(src, sh, dst, dh)
    return ctx.icp_linearize(src, sh, dst, dh, ph, T, max_dist, max_edge)


@pytest.fixture(scope="module")
def wall():
    xyz, has, ph = M.wall_target(WW, WH)
    return xyz, has, ph, _dev(xyz, has)


def _wall_points(rng, n):
    """n wall points over the whole grid (the border pixels have no normal), delta in {-3..3}/8 (|delta| = 3/8 fails the gate of
    0.25), src_has with holes and bytes other than 1 -> (src, src_has, keep)"""
    pi, pj, dl = rng.integers(0, WH, n), rng.integers(0, WW, n), rng.integers(-3, 4, n)
    sh = (rng.integers(0, 4, n) * rng.integers(1, 86, n)).astype(np.uint8)
    keep = (pi > 0) & (pi < WH - 1) & (pj > 0) & (pj < WW - 1) & (sh != 0) & (np.abs(dl) <= 2)
    return M.wall_source(WW, WH, pi, pj, dl), sh, keep


def _check_wall(ctx, wall, src, sh, keep, orders=("given", "reversed", "permuted"), seed=0):
    xyz, has, ph, dwall = wall
    cs, cn, _ = M.wall_sums(src, keep)                 # asserts every term on the 1/64 lattice, sum of |terms| below 2^53 / 64
    perm = np.random.default_rng(seed).permutation(len(src))
    for order in orders:
        s, h = {"given": (src, sh), "reversed": (src[::-1], sh[::-1]),
                "permuted": (src[perm], sh[perm])}[order]
        s, h = s.copy(), h.copy()
        for device in (False, True):
            if device:
                gs, gn = ctx.icp_linearize(*_dev(s, h), *dwall, ph, np.eye(3, 4), 0.25, 10.0)
            else:
                gs, gn = ctx.icp_linearize(s, h, xyz, has, ph, np.eye(3, 4), 0.25, 10.0)
            assert gn == cn and bits_equal(gs, cs), (len(src), order, device, gn, cn, np.nonzero(gs != cs))
    return cs, cn


@pytest.mark.parametrize("n", SWEEP)
def test_wall_sums_are_exact_at_every_size_order_and_memory_kind(ctx, wall, n):
    rng = np.random.default_rng(n)
    src, sh, keep = _wall_points(rng, n)
    for k in (0, n - 1):                               # at least one inlier, at both ends
        src[k] = M.wall_source(WW, WH, [1 + k % (WH - 2)], [1 + k % (WW - 2)], [k % 5 - 2])[0]
        sh[k], keep[k] = 255, True
    cs, cn = _check_wall(ctx, wall, src, sh, keep, seed=n)
    assert cn >= min(n, 2) and (n < 1000 or cn > 0.3 * n)


def _rejects(rng, n):
    """n wall points that every rule rejects in turn: a hole in src_has, a border pixel, the gate, a non-finite coordinate, q_z < 0"""
    pi, pj = rng.integers(1, WH - 1, n), rng.integers(1, WW - 1, n)
    kind = rng.integers(0, 5, n)
    pj = np.where(kind == 1, rng.choice([0, WW - 1], n), pj)
    src = M.wall_source(WW, WH, pi, pj, np.where(kind == 2, rng.choice([-3, 3], n), 1))
    sh = np.where(kind == 0, 0, 1 + rng.integers(0, 255, n)).astype(np.uint8)
    bad = kind == 3
    src[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), int(bad.sum()))
    src[kind == 4, 2] *= -1
    return src, sh


@pytest.mark.parametrize("n", [65, 1025, 262145, 5 * 262144 + 777])
def test_wall_sums_are_exact_with_inliers_planted_at_the_tree_edges(ctx, wall, n):
    """every slot a reject but a few inliers at index 0, n - 1, and the wave, workgroup and grid-stride boundaries"""
    rng = np.random.default_rng(n + 1)
    src, sh = _rejects(rng, n)
    G = min(-(-n // 1024), 256)
    stride = G * 1024
    at = {0, n - 1, 63, 64, 1023, 1024, 1025, 2047, stride - 1, stride, stride + 1, 2 * stride - 1, (G - 1) * 1024, n - 2}
    at = sorted(k for k in at if 0 <= k < n)
    keep = np.zeros(n, bool)
    keep[at] = True
    pi, pj = 1 + rng.integers(0, WH - 2, len(at)), 1 + rng.integers(0, WW - 2, len(at))
    src[at] = M.wall_source(WW, WH, pi, pj, rng.integers(-2, 3, len(at)))
    sh[at] = rng.integers(1, 256, len(at))
    cs, cn = _check_wall(ctx, wall, src, sh, keep, orders=("given", "reversed"))
    assert cn == len(at)


def test_sums_are_within_the_rounding_bound_on_an_anisotropic_scene(ctx):
    W, H = 1024, 768
    ph = _anisotropic(W, H)
    xa, ha = M.render(W, H, ph)
    xb, hb = M.render(W, H, ph, M.motion())
    nrm, nv = M.normals(xa, ha, 10.0)
    T = M.invert(M.motion(axis=(-0.2, 1.0, 0.4), deg=1.2, t=(1.5, -2.0, 1.0)))
    terms, en = M.linearize_terms(xb, hb, xa, ha, nrm, nv, ph, T, 30.0)
    for device in (False, True):
        gs, gn = _lin(ctx, xb, hb, xa, ha, ph, T, 30.0, device)
        assert gn == en > 0.6 * W * H, (gn, en)
        M.assert_within_rounding_bound(gs, terms, W * H)
    # fx and fy are not interchangeable here (every other fixture has fx == fy)
    assert _lin(ctx, xb, hb, xa, ha, (ph[1], ph[0], ph[2], ph[3]), T, 30.0)[1] < 0.5 * en


# ---- projection and gate edges: a 64 x 48 wall, T = identity, every quantity dyadic ------------------------------------------------
EW, EH = 64, 48


def _edge_case(ctx, src, dst_has, max_dist=1.0, T=None, q=None, expect=None):
    """linearise src against the small wall with the given holes; count and sums must equal the model and the closed form (over
    `expect`: the indices that are kept, with q the transformed points if T is not the identity)"""
    xyz, _, ph = M.wall_target(EW, EH)
    src = np.ascontiguousarray(np.asarray(src, np.float32).reshape(-1, 3))
    T = np.eye(3, 4) if T is None else T
    nrm, nv = M.normals(xyz, dst_has, 10.0)
    es, en = M.linearize(src, None, xyz, dst_has, nrm, nv, ph, T, max_dist)
    keep = np.zeros(len(src), bool)
    keep[list(expect or [])] = True
    cs, cn = M.wall_sums_fraction(src if q is None else q, keep)
    for device in (False, True):
        gs, gn = _lin(ctx, src, None, xyz, dst_has, ph, T, max_dist, device)
        assert gn == en == cn and bits_equal(gs, cs) and np.array_equal(gs, es), (gn, en, cn, np.nonzero(gs != cs))
    return cn


def _point(u, v, z=M.WALL_Z):
    """the f32 point that projects (T = identity) to exactly (u, v) on the small wall's pinhole, asserted exact"""
    fx, fy, cx, cy = M.wall_pinhole(EW, EH)
    p = np.float32([(u - cx) * z / fx, (v - cy) * z / fy, z])
    assert float(p[0]) / float(p[2]) * fx + cx == u and float(p[1]) / float(p[2]) * fy + cy == v
    return p


def test_half_pixels_round_up_on_u_and_v(ctx):
    """floor(u + 0.5): u = j + 1/2 takes pixel j + 1, u = j + 1/2 - 2^-20 takes j (and the same on v).  A hole next to one of the
    two candidate pixels takes its normal away, so the count tells which pixel the point went to."""
    i, j, eps = 20, 30, 2.0 ** -20
    for axis in "uv":
        lo, hi = ((i, j), (i, j + 1)) if axis == "u" else ((i, j), (i + 1, j))
        beyond_lo = (lo[0], lo[1] - 1) if axis == "u" else (lo[0] - 1, lo[1])
        beyond_hi = (hi[0], hi[1] + 1) if axis == "u" else (hi[0] + 1, hi[1])
        for frac, lands in ((0.5, hi), (0.5 - eps, lo)):
            p = _point(j + frac, i) if axis == "u" else _point(j, i + frac)
            for hole, dead in ((beyond_lo, lo), (beyond_hi, hi)):
                has = np.ones((EH, EW), np.uint8)
                has[hole] = 0
                n = _edge_case(ctx, p, has, expect=[0] if lands != dead else [])
                assert n == (0 if lands == dead else 1), (axis, frac, hole)


def test_gate_keeps_equality(ctx):
    has = np.ones((EH, EW), np.uint8)
    p = _point(30, 20)
    gz = p + np.float32([0, 0, 0.375])                                  # |d| = 3/8
    g345 = _point(30.375, 20) + np.float32([0, 0, 0.5])                 # d = (3/8, 0, 1/2): |d| = 5/8
    for src, dist in ((gz, 0.375), (g345, 0.625)):
        below = math.nextafter(dist, 0)
        assert below * below < dist * dist
        assert _edge_case(ctx, src, has, max_dist=dist, expect=[0]) == 1
        assert _edge_case(ctx, src, has, max_dist=below) == 0


def test_degenerate_points_are_rejected(ctx):
    """q_z of 0, -0 and below, a denormal z, |u| or |v| beyond 2^31 (2^32 off a valid pixel: an int conversion before the range
    check would wrap onto the grid), an infinite u, and NaN / +-inf in each coordinate, between kept points"""
    has = np.ones((EH, EW), np.uint8)
    fx, fy, cx, cy = M.wall_pinhole(EW, EH)
    good = [_point(10, 10), _point(40, 30)]
    den = np.float32(1e-40)
    bad = [(1, 1, 0), (1, 1, -0.0), (1, 1, -1024), (1, 1, -1e-45), (1, 1, den), (0, 0, den), (-1e30, 1, den),
           (2.0 ** 31, 0, 1024), (-2.0 ** 31, 0, 1024), (2.0 ** 32, 0, 1024), (-2.0 ** 32, 0, 1024), (2.0 ** 40, 0, 1024),
           (0, 2.0 ** 32, 1024), (0, 2.0 ** 33, 1024), (0, -2.0 ** 33, 1024), (0, 2.0 ** 34, 1024)]
    for c in range(3):
        for x in (np.nan, np.inf, -np.inf):
            p = list(_point(31, 21))
            p[c] = x
            bad.append(tuple(p))
    src = np.float32(good + bad)
    assert _edge_case(ctx, src, has, expect=[0, 1]) == 2
    # q_z = -0: every product and addend of the third row -0
    T = np.eye(3, 4)
    T[2, 3] = -0.0
    mz = np.float32([[-1, -1, -0.0], [-3, -2, -0.0]])
    assert math.copysign(1, ((T[2, 0] * -1.0 + T[2, 1] * -1.0) + T[2, 2] * -0.0) + T[2, 3]) == -1
    assert _edge_case(ctx, np.concatenate([np.float32(good), mz]), has, T=T, q=np.float32(good + [[0, 0, 0]] * 2), expect=[0, 1]) == 2
    # a T that overflows q_x: u = inf
    Tb = np.eye(3, 4)
    Tb[0, 0] = 1e300
    assert _edge_case(ctx, np.float32([[1, 1, 1024], [-1, 1, 1024]]), has, T=Tb) == 0
    # a T with zero coefficients: q_z = 1024 whatever z is, and still a non-finite z or y rejects the point
    Tz = np.array([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1024]])
    zs = np.float32([_point(12, 9)[:2].tolist() + [5.0], _point(50, 40)[:2].tolist() + [-7.0]])
    nf = np.float32([[zs[0, 0], zs[0, 1], np.nan], [zs[0, 0], zs[0, 1], np.inf], [zs[0, 0], np.inf, 3.0], [np.nan, zs[0, 1], 1.0]])
    q = np.concatenate([zs, nf]).copy()
    q[:, 2] = M.WALL_Z
    assert _edge_case(ctx, np.concatenate([zs, nf]), has, T=Tz, q=q, expect=[0, 1]) == 2


# ---- the registration loop ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aniso_pair():
    W, H = 320, 240
    ph = _anisotropic(W, H)
    xa, ha = M.render(W, H, ph)
    xb, hb = M.render(W, H, ph, M.motion())
    return ph, xa, ha, xb, hb


def test_one_step_is_the_host_solve_and_update_bit_for_bit(ctx, aniso_pair):
    ph, xa, ha, xb, hb = aniso_pair
    T0 = M.invert(M.motion(deg=1.1, t=(1.5, -2.0, 2.0))).astype(np.float32)
    for T_init in (T0, None):
        T64 = np.eye(3, 4) if T_init is None else T_init.astype(np.float64)
        gs, gn = ctx.icp_linearize(xb, hb, xa, ha, ph, T64, 40.0, 10.0)
        T, res = ctx.register_icp(xb, hb, xa, ha, ph, T_init=T_init, max_dist=40.0, max_iters=1)
        xi = M.solve(gs)
        assert res["iterations"] == 1 and res["stop_reason"] == 2 and res["inliers"] == gn > 0.5 * xa.shape[0] * xa.shape[1], res
        assert bits_equal(res["T64"], M.update_exact(xi, T64)) and bits_equal(T, res["T64"].astype(np.float32))
        assert bits_equal(np.float64(res["rms"]), np.float64(math.sqrt(gs[27] / gn)))
    # from identity the translation column is v itself; xi against the rational solve of the same A and b
    assert bits_equal(res["T64"][:, 3], xi[3:])
    err, kappa = M.solve_error(gs, xi)
    assert err <= 8 * kappa * U and np.linalg.norm(xi[3:]) > 1.0, (err, kappa)


def test_max_iters_stops_with_reason_2(ctx, aniso_pair):
    """stop_rot = stop_trans = 0: never converged.  The loop replayed step by step from the GPU's own linearisations, bit for bit"""
    ph, xa, ha, xb, hb = aniso_pair
    n_it = 5
    T, res = ctx.register_icp(xb, hb, xa, ha, ph, max_dist=40.0, max_iters=n_it, stop_rot=0.0, stop_trans=0.0)
    assert res["stop_reason"] == 2 and res["iterations"] == n_it, res
    Tr = np.eye(3, 4)
    for _ in range(n_it):
        gs, gn = ctx.icp_linearize(xb, hb, xa, ha, ph, Tr, 40.0, 10.0)
        Tr = M.update_exact(M.solve(gs), Tr)
    assert bits_equal(res["T64"], Tr)
    assert res["inliers"] == gn and bits_equal(np.float64(res["rms"]), np.float64(math.sqrt(gs[27] / gn)))
    ET, eres = M.register(xb, hb, xa, ha, ph, max_dist=40.0, max_iters=n_it, stop_rot=0.0, stop_trans=0.0)
    assert eres["stop_reason"] == 2 and eres["iterations"] == n_it and eres["inliers"] == res["inliers"]
    assert np.abs(res["T64"] - ET).max() < 1e-7


def test_min_inliers_at_its_boundary(ctx, wall):
    """on the wall, where the inlier count N is known exactly: min_inliers = N gets past the count (and the plane is singular),
    N + 1 stops with reason 3 before any update"""
    xyz, has, ph, dwall = wall
    src, sh, keep = _wall_points(np.random.default_rng(5), 100000)
    cs, N, _ = M.wall_sums(src, keep)
    T0 = np.eye(3, 4, dtype=np.float32)
    for device in (False, True):
        args = (*_dev(src, sh), *dwall) if device else (src, sh, xyz, has)
        T, res = ctx.register_icp(*args, ph, T_init=T0, max_dist=0.25, min_inliers=N)
        assert res["stop_reason"] == 4 and res["iterations"] == 0 and res["inliers"] == N, res
        T, res = ctx.register_icp(*args, ph, T_init=T0, max_dist=0.25, min_inliers=N + 1)
        assert res["stop_reason"] == 3 and res["iterations"] == 0 and res["inliers"] == N, res
        assert bits_equal(T, T0) and bits_equal(res["T64"], T0.astype(np.float64))
        assert bits_equal(np.float64(res["rms"]), np.float64(math.sqrt(cs[27] / N)))


def test_singular_beyond_the_plane(ctx):
    """a sphere (free twists about its centre) and two planes (a free translation along their line) are singular; a three-plane
    corner is not and converges as the model does"""
    W, H = 320, 240
    ph = _anisotropic(W, H)
    A = M.motion()
    walls = [("plane", (0.0, 0.0, -1.0), -1250.0), ("plane", (0.8, 0.0, -0.6), -900.0)]
    scenes = {"sphere": ([], [((0.0, 0.0, 1000.0), 300.0)]), "two planes": (walls, []),
              "corner": (walls + [("plane", (0.0, -1.0, 0.0), -260.0)], [])}
    for name, scene in scenes.items():
        xa, ha = M.render(W, H, ph, scene=scene)
        xb, hb = M.render(W, H, ph, A, scene=scene)
        T, res = ctx.register_icp(xb, hb, xa, ha, ph, max_dist=40.0)
        ET, eres = M.register(xb, hb, xa, ha, ph, max_dist=40.0)
        assert res["inliers"] > 10000 and {k: res[k] for k in ("iterations", "stop_reason", "inliers")} == \
            {k: eres[k] for k in ("iterations", "stop_reason", "inliers")}, (name, res, eres)
        if name == "corner":
            assert res["stop_reason"] == 1 and res["iterations"] >= 2 and np.abs(res["T64"] - ET).max() < 1e-7, (name, res)
        else:
            assert res["stop_reason"] == 4 and res["iterations"] == 0 and bits_equal(T, np.eye(3, 4, dtype=np.float32)), (name, res)


def test_empty_source(ctx, slr, wall):
    """n_src = 0 (include/slr.h): null source pointers allowed, zero sums written over the poisoned scratch, stop reason 3"""
    xyz, has, ph, dwall = wall
    T0 = M.motion(deg=0.5, t=(1.0, 0.0, 0.0)).astype(np.float32)
    empties = [(np.zeros((0, 3), np.float32), None, xyz, has), (np.zeros((0, 3), np.float32), np.zeros(0, np.uint8), xyz, has),
               (torch.empty((0, 3), device="cuda"), None, *dwall),
               (torch.empty((0, 3), device="cuda"), torch.empty(0, dtype=torch.uint8, device="cuda"), *dwall)]
    for args in empties:
        ctx.icp_linearize(M.wall_source(WW, WH, [5, 6], [7, 8], [1, -1]), None, xyz, has, ph, np.eye(3, 4), 0.25, 10.0)  # real sums first
        gs, gn = ctx.icp_linearize(*args, ph, np.eye(3, 4), 0.25, 10.0)
        assert gn == 0 and bits_equal(gs, np.zeros(28)), gs
        T, res = ctx.register_icp(*args, ph, T_init=T0, max_dist=0.25)
        assert (res["stop_reason"], res["iterations"], res["inliers"], res["rms"]) == (3, 0, 0, 0.0), res
        assert bits_equal(T, T0)
    # the C ABI with NULL source pointers on host memory
    D = slr.capi.IcpDesc
    d = D(WW, WH, *ph, 0.25, 10.0, 1, 0.0, 0.0, 6)
    sums, n = np.full(28, 7.0), C.c_uint64(9)
    Th = np.eye(3, 4).reshape(12)
    assert ctx.lib.slr_icp_linearize(ctx.h, C.byref(d), None, None, C.c_size_t(0), C.c_void_p(xyz.ctypes.data),
                                     C.c_void_p(has.ctypes.data), C.c_void_p(Th.ctypes.data), C.c_void_p(sums.ctypes.data),
                                     C.byref(n), C.c_int(slr.capi.MEM_HOST)) == slr.capi.OK
    assert n.value == 0 and bits_equal(sums, np.zeros(28))
    # ... but not with points to read
    assert ctx.lib.slr_icp_linearize(ctx.h, C.byref(d), None, None, C.c_size_t(1), C.c_void_p(xyz.ctypes.data),
                                     C.c_void_p(has.ctypes.data), C.c_void_p(Th.ctypes.data), C.c_void_p(sums.ctypes.data),
                                     C.byref(n), C.c_int(slr.capi.MEM_HOST)) == slr.capi.ERR_INVALID_ARG

