"""bench.py --dump-outputs: the last timed step's XYZ + mask written as .npy, so that two builds can be compared output for output.
CPU half: the writer itself (every pixel of a small output, a fixed seeded sample of a large one).  GPU half: a short bench run whose
dump must equal, bit for bit, the single-frame entry on the same seeded frames and rig, with --steps honoured in the line."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLACK = 40


def _bench_module():
    """bench.py as a module.  Importing it drops the suite's poison switches (tests/conftest.py) from os.environ; they are put
    back, or every later import of the package and every child process of the suite would run without them."""
    saved = {k: os.environ[k] for k in ("SLR_POISON_OUTPUTS", "SLR_POISON_SCRATCH") if k in os.environ}
    try:
        spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
        bench = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bench)
    finally:
        os.environ.update(saved)
    return bench


def _load(d):
    return [np.load(os.path.join(str(d), n + ".npy")) for n in ("xyz", "has", "pixel_index")]


def test_dump_outputs_writes_every_pixel_of_a_small_output_in_frame_order(tmp_path):
    bench = _bench_module()
    x0 = torch.arange(2 * 3 * 4 * 3, dtype=torch.float32).reshape(2, 3, 4, 3)
    h0 = (torch.arange(24, dtype=torch.uint8) % 2).reshape(2, 3, 4)
    x1, h1 = x0 + 1000, h0 ^ 1
    bench.dump_outputs(str(tmp_path), [(x0, h0), (x1, h1)])
    xyz, has, idx = _load(tmp_path)
    assert (xyz.dtype, has.dtype, idx.dtype) == (np.float32, np.float32, np.float64)
    assert np.array_equal(xyz, torch.cat([x0.reshape(-1, 3), x1.reshape(-1, 3)]).numpy())
    assert np.array_equal(has, torch.cat([h0.reshape(-1), h1.reshape(-1)]).numpy().astype(np.float32))
    assert np.array_equal(idx, np.arange(48))


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(tmp_path):
    bench = _bench_module()
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 700, 600, 3), generator=g)
    h = (torch.rand((3, 700, 600), generator=g) > 0.5).to(torch.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [(x[:2], h[:2]), (x[2:], h[2:])])
    xyz, has, idx = _load(tmp_path / "a")
    sel = idx.astype(np.int64)
    assert len(sel) == bench.DUMP_SAMPLE and np.all(np.diff(sel) > 0) and sel[-1] < x.shape[0] * 700 * 600
    assert np.array_equal(xyz, x.reshape(-1, 3).numpy()[sel])
    assert np.array_equal(has, h.reshape(-1).numpy()[sel].astype(np.float32))
    assert all(np.array_equal(a, b) for a, b in zip(_load(tmp_path / "a"), _load(tmp_path / "b")))
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a"))) <= 64 << 20


@pytest.mark.gpu
def test_bench_dump_is_what_the_timed_path_computed(slr, synth, tmp_path):
    """1024x512, 2 frames on bench.py's default rig (verged by 0.2 rad): 2 x 1024 x 512 pixels = DUMP_SAMPLE, so every pixel is
    written; each frame must equal slr_reconstruct_mf on the same seeded planes."""
    W, H, F, STEPS = 1024, 512, 2, 3
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--frames", str(F),
           "--width", str(W), "--height", str(H), "--traffic", "off", "--cpu-baseline", "0", "--host-io", "0", "--map-sweep", "0",
           "--both-models", "0", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    xyz, has, idx = _load(out)
    assert np.array_equal(idx, np.arange(F * H * W))
    rig = synth.make_verged_rig(W, H, 0.2, -0.15)
    c = slr.Context(0)
    try:
        c.set_calibration(rig["calib"])
        synth.install_verged_maps(c, rig, W, H)
        dev = torch.device("cuda", 0)
        for f in range(F):
            st = synth.render_mf_stack(W, H, seed=1234 + f, noise=2, device=dev)
            ex, eh = c.reconstruct_mf(st[0], st[1], BLACK, True, W=W)
            c.synchronize()
            sl = slice(f * H * W, (f + 1) * H * W)
            assert bits_equal(xyz[sl], ex.cpu().numpy().reshape(-1, 3)), f
            assert np.array_equal(has[sl], eh.cpu().numpy().reshape(-1).astype(np.float32)), f
        assert has.any()
    finally:
        c.close()
