"""The host mirror's fused scan series: `slr_cli <project> mf --series K --fuse VOXEL --min-points N` on a synthetic project in
the reference's layout writes reconstruction/fused.ply, whose vertices are the NumPy model (tests/np_fuse_model.py) applied to
the per-scan PointCloudImage clouds (each point sum / count as slr_pointcloud_get forms it, every scan already moved by its
transfer_mat), in the mesh writer's number format; duke_fuse_series gives the same points bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_fuse_model as M
from test_host_mirror import _p, _write_project, host  # noqa: F401  (host: the libslr_host.so fixture)
from util import bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "structure-light-reconstructor_amd", "slr_cli")


def _expected_ply(pts):
    s = "ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(pts)
    return s + "".join("%g %g %g\n" % (float(p[0]), float(p[1]), float(p[2])) for p in pts)


def test_cli_series_fuse_writes_the_model(host, slr, synth, tmp_path):
    W, H, scan_w, scan_h, n = 320, 96, 200, 340, 3
    calib, _ = synth.make_calibration(W, H, baseline=400.0, theta=0.6)
    proj = None
    for sn in range(n):
        proj = _write_project(host, tmp_path, synth, W, H, calib, synth.render_mf_stack(W, H, seed=90 + sn).numpy(), sn=sn)
    for sn in (1, 2):
        Tm = np.array([[1, 0, 0, 3.0 * sn], [0, 1, 0, -1.5], [0, 0, 1, 0.25 * sn]], np.float64)
        assert host.duke_export_mat(os.path.join(proj, "scan/transfer_mat%d.txt" % sn).encode(), _p(Tm), 3, 4) == 1
    voxel, min_points = 2.0, 2
    r = subprocess.run([CLI, proj, "mf", "--series", str(n), "--scan", str(scan_w), str(scan_h), "--cam", str(W), str(H),
                        "--fuse", "%g" % voxel, "--min-points", str(min_points)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fused = os.path.join(proj, "reconstruction", "fused.ply")
    for sn in range(n):
        assert os.path.exists(os.path.join(proj, "reconstruction", "%d.ply" % sn))     # the per-scan meshes as before
    # the per-scan clouds of the same series, and the model applied to them
    err = C.create_string_buffer(512)
    ss = np.zeros((n, scan_h, scan_w, 3), np.float32)
    sc = np.zeros((n, scan_h, scan_w), np.uint8)
    assert host.duke_run_series(proj.encode(), 0, n, scan_w, scan_h, W, H, 40, 0, b".png", None, _p(ss), _p(sc), err, 512) == n, err.value
    ctx = slr.Context(0)
    pts = ctx.pointcloud_get(ss, sc)
    ctx.close()
    ex, ec, _, rej = M.fuse(pts, sc, voxel, min_points=min_points)
    assert len(ec) > 20 and (ec > 2).any()            # (a few far-off triangulations are rejected: the model counts them too)
    assert open(fused).read() == _expected_ply(ex)
    # duke_fuse_series hands the fused points over as floats: bit for bit
    out = np.zeros((n * scan_h * scan_w, 3), np.float32)
    m = C.c_uint32(0)
    other = os.path.join(proj, "reconstruction", "fused_again.ply")
    host.duke_fuse_series.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                      C.c_char_p, C.c_void_p, C.c_int, C.c_double, C.c_uint, C.c_char_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    assert host.duke_fuse_series(proj.encode(), 0, n, scan_w, scan_h, W, H, 40, 0, b".png", None, None, 0, voxel, min_points,
                                 other.encode(), None, None, _p(out), C.addressof(m), err, 512) == 1, err.value
    assert m.value == len(ec) and bits_equal(out[:m.value], ex)
    assert open(other).read() == open(fused).read()
    # --fuse without a series is refused
    r = subprocess.run([CLI, proj, "mf", "--fuse", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
