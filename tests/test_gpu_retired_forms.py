"""The retired kernel forms: their option values still pass the range checks, answer SLR_ERR_UNSUPPORTED and
leave the option at its previous value -- the previous form is the one that keeps running."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BLACK = 40
RETIRED_RECT_DECODE_ALGOS = (2, 3, 4)
RETIRED_RECT_DMA_SHAPES = (2, 4, 5, 6)
RETIRED_MF_MATCH_ALGOS = (2, 5, 6, 7, 9)


def _refused(ctx, slr, opt, value):
    with pytest.raises(slr.capi.SlrError) as ei:
        ctx.set_option(opt, value)
    assert ei.value.status == slr.capi.ERR_UNSUPPORTED, (opt, value, str(ei.value))


def test_retired_decode_forms_and_dma_shapes_keep_the_previous_value(ctx, slr, synth):
    W, H = 256, 64
    for cam in range(2):
        mx, mf = synth.make_rectify_maps(W, H, cam)
        ctx.set_rectify_maps(cam, mx.numpy(), mf.numpy())
    try:
        for prev in (5, 6, 1):
            ctx.set_option(slr.capi.OPT_RECT_DECODE_ALGO, prev)
            for value in RETIRED_RECT_DECODE_ALGOS:
                _refused(ctx, slr, slr.capi.OPT_RECT_DECODE_ALGO, value)
                assert [ctx.rectify_info(cam)["mf_form"] for cam in range(2)] == [prev, prev], (prev, value)
        for prev in (0, 1, 3):
            ctx.set_option(slr.capi.OPT_RECT_DMA_SHAPE, prev)
            for value in RETIRED_RECT_DMA_SHAPES:
                _refused(ctx, slr, slr.capi.OPT_RECT_DMA_SHAPE, value)
                assert [ctx.rectify_info(cam)["dma_shape"] for cam in range(2)] == [prev, prev], (prev, value)
    finally:
        ctx.set_option(slr.capi.OPT_RECT_DECODE_ALGO, 0)
        ctx.set_option(slr.capi.OPT_RECT_DMA_SHAPE, 3)


def test_retired_match_forms_keep_the_previous_value(ctx, slr, synth):
    """the lean K4 matches the frames of a batch group in one launch, the general binned form frame by frame: the frames that the
    first match launch of a batch served (the profiler samples only that launch) tell which of the two still runs after a retired
    value was refused"""
    W, H, frames = 2052, 9, 3
    calib, _ = synth.make_calibration(W, H, with_T=True)
    ctx.set_calibration(calib)
    for cam in range(2):
        mx, mf = synth.make_rectify_maps(W, H, cam)
        ctx.set_rectify_maps(cam, mx.numpy(), mf.numpy())
    stack = torch.stack([synth.render_mf_stack(W, H, seed=500 + f, noise=2) for f in range(frames)]).cuda()

    def frames_of_first_match_launch():
        ctx.profile_reset()
        ctx.reconstruct_mf_batch(stack, BLACK, True)
        ctx.synchronize()
        return ctx.profile()["slr_mf_match_triangulate"][1]

    ctx.set_option(slr.capi.OPT_PROFILE_STRIDE, 1 << 20)
    ctx.profile_enable(True)
    try:
        for prev, want in ((0, frames), (3, 1)):
            ctx.set_option(slr.capi.OPT_MF_MATCH_ALGO, prev)
            assert frames_of_first_match_launch() == want, prev
            for value in RETIRED_MF_MATCH_ALGOS:
                _refused(ctx, slr, slr.capi.OPT_MF_MATCH_ALGO, value)
                assert frames_of_first_match_launch() == want, (prev, value)
    finally:
        ctx.profile_enable(False)
        ctx.set_option(slr.capi.OPT_PROFILE_STRIDE, 1)
        ctx.set_option(slr.capi.OPT_MF_MATCH_ALGO, 0)
