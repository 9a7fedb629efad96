"""Visits of several frames in the grouped fused decode (kernels_rectdma.hip, VISITS): slr_reconstruct_mf_batch decodes each tile
for up to kDmaVisitFrames frames of a camera back to back, with the tap setup and the digest fetch once per visit.
SLR_OPT_DEBUG_FLAGS bit 10 keeps one frame per visit.  Both must give the same clouds, bit for bit, and the same as single-frame
slr_reconstruct_mf calls:

* group sizes 1, 3, 5 and 8 (the sets of a group are not always full);
* stereo heads verged by 0.2 rad (bench.py's maps) and 0.3 rad at 4096x3000 (tiles decoded in parts; the gather fix-up of tiles
  no split makes fit where there are any) and near-identity maps, the latter also on few workgroups (many visits per workgroup);
* both evaluation models;
* with the scratch poisoned, so a frame whose phases were never written cannot pass for another's.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
BLACK = 40


def _frames(synth, W, H, n):
    dev = torch.device("cuda", 0)
    st = torch.stack([synth.render_mf_stack(W, H, seed=77 + f, noise=2, device=dev) for f in range(n)])
    torch.cuda.synchronize()
    return st


def _batch(ctx, slr, frames, flags):
    ctx.set_option(slr.capi.OPT_DEBUG_FLAGS, flags)
    try:
        xyz, has = ctx.reconstruct_mf_batch(frames, BLACK, True)
        ctx.synchronize()
    finally:
        ctx.set_option(slr.capi.OPT_DEBUG_FLAGS, 0)
    return xyz, has


def _check(ctx, slr, frames):
    """every group size: visits == one frame per visit == single-frame calls, XYZ and mask bytes"""
    single = []
    for f in range(frames.shape[0]):
        x, h = ctx.reconstruct_mf(frames[f, 0], frames[f, 1], BLACK, True)
        ctx.synchronize()
        single.append((x.clone(), h.clone()))
    for g in (1, 3, 5, 8):
        xv, hv = _batch(ctx, slr, frames[:g], 0)
        x1, h1 = _batch(ctx, slr, frames[:g], slr.capi.DEBUG_ONE_FRAME_VISITS)
        for f in range(g):
            assert torch.equal(hv[f], h1[f]) and torch.equal(hv[f], single[f][1]), (g, f)
            assert torch.equal(xv[f].view(torch.int32), x1[f].view(torch.int32)), (g, f)
            assert torch.equal(xv[f].view(torch.int32), single[f][0].view(torch.int32)), (g, f)
        assert hv.float().mean().item() > 0.2, g


@pytest.fixture(params=[0, 1], ids=["strict", "x87"])
def model_ctx(request, slr):
    c = slr.Context(0)
    c.set_option(slr.capi.OPT_DEBUG_POISON_SCRATCH, 1)
    if request.param:
        c.set_option(slr.capi.OPT_EVAL_MODEL, 1)
    yield c
    c.close()


@pytest.mark.parametrize("theta,k1", [(0.2, -0.15), (0.3, -0.2)])
def test_visits_on_the_verged_rig(slr, synth, model_ctx, theta, k1):
    W, H = 4096, 3000
    ctx = model_ctx
    rig = synth.make_verged_rig(W, H, theta, k1)
    ctx.set_calibration(rig["calib"])
    synth.install_verged_maps(ctx, rig, W, H)
    info = [ctx.rectify_info(cam) for cam in range(2)]
    print("verged rig theta %.1f k1 %.2f:" % (theta, k1), info)
    assert all(i["mf_form"] == 7 for i in info), info
    assert sum(i["dma_extra_entries"] for i in info) > 0, info                 # (tiles decoded in parts)
    _check(ctx, slr, _frames(synth, W, H, 8))


@pytest.mark.parametrize("resident", [0, 64])
def test_visits_on_near_identity_maps(slr, synth, model_ctx, resident):
    W, H = 1024, 768
    ctx = model_ctx
    calib, _ = synth.make_calibration(W, H, with_T=True)
    ctx.set_calibration(calib)
    for cam in range(2):
        mx, mf = synth.make_rectify_maps(W, H, cam)
        ctx.set_rectify_maps(cam, mx.numpy(), mf.numpy())
    assert all(ctx.rectify_info(cam)["mf_form"] == 7 for cam in range(2))
    ctx.set_option(slr.capi.OPT_DEBUG_RECT_RESIDENT, resident)     # 64 workgroups: many visits per workgroup
    try:
        _check(ctx, slr, _frames(synth, W, H, 8))
    finally:
        ctx.set_option(slr.capi.OPT_DEBUG_RECT_RESIDENT, 0)
