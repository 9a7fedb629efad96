"""The host mirror's registered scan series: `slr_cli <project> mf --series 2 --fuse VOXEL --register MAX_DIST` on a synthetic project
whose scan 1 holds scan 0's images under a perturbed transfer_mat1.  A small perturbation (0.1 deg, 0.8 mm) is undone: the correction is
applied, reconstruction/transfer_mat1.txt (correction o original, in that order) comes out at identity and the two scans fuse into
fewer cells than without --register.  A large one with a wide gate (1 deg, 4.9 mm, 500 mm), from which the unweighted loop drifts on
these terraced K4 clouds, is not applied: the scan keeps its transfer_mat and the fusion is the one without --register."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import np_icp_model as M
from test_host_mirror import _p, host  # noqa: F401  (host: the libslr_host.so fixture)
from util import bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "structure-light-reconstructor_amd", "slr_cli")


def _write_rectified_project(host, root, W, H, stack, n_scans):
    """a project whose calibration is already rectified (no distortion, parallel cameras 120 mm apart), so the synthetic stacks'
    disparities triangulate to a smooth surface: a tilted plane with a bump, 1.5 to 7 m away"""
    f, cx, cy = 1.2 * W, 0.5 * W, 0.5 * H
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]])

    def put(rel, arr):
        a = np.ascontiguousarray(np.asarray(arr, np.float64))
        a2 = a.reshape(a.shape[0], -1)
        assert host.duke_export_mat(os.path.join(root, rel).encode(), _p(a2), a2.shape[0], a2.shape[1]) == 1
    for d in ("calib/left", "calib/right", "reconstruction"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for side in ("left", "right"):
        put("calib/%s/cam_matrix.txt" % side, K)
        put("calib/%s/cam_distortion.txt" % side, np.zeros((5, 1)))
        put("calib/%s/cam_rotation_matrix.txt" % side, np.eye(3))
        put("calib/%s/cam_trans_vectror.txt" % side, np.zeros((3, 1)) if side == "left" else np.array([[-120.0], [0.0], [0.0]]))
        put("calib/%s/cam_stereo.txt" % side, K)
        put("calib/%s/distortion_stereo.txt" % side, np.zeros((5, 1)))
    put("calib/R_stereo.txt", np.eye(3))
    put("calib/T_stereo.txt", np.array([[-120.0], [0.0], [0.0]]))
    put("calib/fundamental_stereo.txt", np.eye(3))
    put("calib/H1_mat.txt", np.eye(3)); put("calib/H2_mat.txt", np.eye(3))
    for sn in range(n_scans):
        for cam, side, pre in ((0, "left", "L"), (1, "right", "R")):
            os.makedirs(os.path.join(root, "scan/%s/%d" % (side, sn)), exist_ok=True)
            for i in range(stack.shape[1]):
                path = os.path.join(root, "scan/%s/%d/%s%d.png" % (side, sn, pre, i)).encode()
                assert host.duke_imwrite(path, _p(np.ascontiguousarray(stack[cam, i])), W, H, 1) == 1


def _vertices(path):
    return int(re.search(r"element vertex (\d+)", open(path).read(200)).group(1))


def _off_identity(T):
    T = np.asarray(T, np.float64).reshape(3, 4)
    return np.degrees(np.arccos(np.clip((np.trace(T[:, :3]) - 1) / 2, -1, 1))), np.abs(T[:, 3]).max()


def _compose(A, B):
    """A o B for 3x4 transforms, in the host mirror's operation order (f64)"""
    A, B = np.asarray(A, np.float64).reshape(3, 4), np.asarray(B, np.float64).reshape(3, 4)
    out = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            v = A[r, 3] if c == 3 else 0.0
            for m in range(3):
                v += A[r, m] * B[m, c]
            out[r, c] = v
    return out


def test_cli_register_undoes_a_small_perturbation_and_refuses_a_drift(host, slr, synth, tmp_path):
    W, H = 640, 240
    scan_w, scan_h = H, W                                 # the PointCloudImage holds the whole camera grid (transposed)
    proj = str(tmp_path)
    _write_rectified_project(host, proj, W, H, synth.render_mf_stack(W, H, seed=90).numpy(), 2)
    tm = os.path.join(proj, "scan/transfer_mat1.txt").encode()
    out = os.path.join(proj, "reconstruction/transfer_mat1.txt")
    fused = os.path.join(proj, "reconstruction", "fused.ply")
    base = [CLI, proj, "mf", "--series", "2", "--scan", str(scan_w), str(scan_h), "--cam", str(W), str(H), "--fuse", "2"]

    def run(*extra):
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout

    # a small perturbation: undone, applied, written as correction o original
    O = M.motion(axis=(0.2, 1.0, -0.3), deg=0.1, t=(0.5, -0.5, 0.3))
    assert host.duke_export_mat(tm, _p(np.ascontiguousarray(O)), 3, 4) == 1
    run()
    plain = _vertices(fused)
    stdout = run("--register", "50")
    assert re.search(r"scan 1: \d+ iterations, \d+ inliers, rms \S+, converged, applied", stdout), stdout
    registered = _vertices(fused)
    assert registered < 0.9 * plain, (registered, plain)
    refined = np.zeros(12, np.float32)
    assert host.duke_load_matrix(out.encode(), 3, 4, _p(refined)) == 1
    O32 = np.zeros(12, np.float32)
    assert host.duke_load_matrix(tm, 3, 4, _p(O32)) == 1                  # the original as the series read it
    ang, dt = _off_identity(refined)
    ang0, dt0 = _off_identity(O32)
    assert ang < 0.01 and dt < 0.05 and ang < ang0 / 10 and dt < dt0 / 10, (ang, dt, ang0, dt0)
    # the order: the library call hands over the correction and the refined matrix; refined = correction o original, bit for bit
    n = 2
    err = C.create_string_buffer(512)
    Tref = np.zeros((n, 12), np.float32)
    res = (slr.capi.IcpResult * n)()
    applied = np.zeros(n, np.int32)
    f = host.duke_register_fuse_series
    f.argtypes = [C.c_char_p] + [C.c_int] * 8 + [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_double, C.c_uint, C.c_char_p, C.c_double,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    again = os.path.join(proj, "reconstruction", "fused_again.ply")
    assert f(proj.encode(), 0, n, scan_w, scan_h, W, H, 40, 0, b".png", None, None, 0, 2.0, 1, again.encode(), 50.0, _p(Tref),
             C.cast(res, C.c_void_p), _p(applied), None, None, err, 512) == 1, err.value
    assert list(applied) == [1, 1] and res[1].stop_reason == 1
    Cr = np.array(list(res[1].T), np.float64)
    assert bits_equal(Tref[1], _compose(Cr, O32).astype(np.float32).reshape(12))
    assert not bits_equal(Tref[1], _compose(O32, Cr).astype(np.float32).reshape(12))
    assert np.abs(Tref[1] - refined).max() < 1e-5                           # the text file: 6 significant digits
    assert open(again).read() == open(fused).read()
    # a large perturbation and a wide gate: the loop drifts, the correction is not applied and the refined matrix is removed
    O = M.motion(axis=(-0.4, 0.9, 0.3), deg=1.0, t=(3.0, -3.5, 1.5))
    assert host.duke_export_mat(tm, _p(np.ascontiguousarray(O)), 3, 4) == 1
    run()
    plain = open(fused).read()
    stdout = run("--register", "500")
    assert re.search(r"scan 1: \d+ iterations, \d+ inliers, rms \S+, \S[^,]*, NOT applied", stdout), stdout
    assert not os.path.exists(out)
    assert open(fused).read() == plain
    assert not os.path.exists(os.path.join(proj, "reconstruction", "transfer_mat0.txt"))
    # refused: a series that does not start at the anchor scan 0, --register without --fuse, a gate <= 0
    for bad in (base + ["--register", "50", "--sn", "1"], base[:-2] + ["--register", "50"], base + ["--register", "-1"]):
        r = subprocess.run(bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--register" in r.stderr, (bad, r.stderr)
