"""Batched multi-scale test on the GPU (HeatmapParser.parse_multi_scale, TeacherPipeline(scale_factors=...),
inference.multi_scale_batch_inference): bit-identical, image by image, to the materialised per-image chain of
rtpe/inference.py multi_scale_inference (get_multi_stage_outputs + aggregate_results per scale on the resize_combine
kernel, / S, then parser.parse), which test_gpu_parity.py pins against the torch restatement of the upstream
protocol."""
import numpy as np
import pytest
import torch

from oracle import synth
from test_flip_decode_gpu import _assert_same, _blob_outputs, _parser

pytestmark = pytest.mark.gpu

J = 17
H, W = 128, 192          # the scale-1 input size of the decode tests


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


@pytest.fixture(scope="module")
def teacher(nat, w48_shapes):
    from rtpe.helpers import build_hrnet_w48_teacher
    sd = synth.make_state_dict(w48_shapes, 0, "W0")
    return build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to("cuda:0")


def _scale_outputs(N, scales, seed):
    """per scale (descending) the blob outputs (P, R, Pf, Rf) of a (H*s, W*s) input"""
    return [_blob_outputs(N, int(H * s), int(W * s), seed=seed + 10 * i) for i, s in enumerate(scales)]


def _materialised(parser, outs, scales, flip, n, adjust=True, refine=True):
    """image n through the per-image chain of multi_scale_inference, with a stand-in model per scale that returns
    the given outputs (the mirrored input gets the mirror image's)"""
    from rtpe import inference
    final, tags_list = None, []
    with torch.no_grad():
        for s, (P, R, Pf, Rf) in zip(scales, outs):
            calls = []

            def model(image):
                calls.append(image)
                return [t[n:n + 1] for t in ((P, R) if len(calls) == 1 else (Pf, Rf))]
            image = torch.zeros((1, 3, 2 * R.shape[2], 2 * R.shape[3]), device="cuda:0")
            _, heatmaps, tags = inference.get_multi_stage_outputs(model, image, flip, True, (W, H))
            assert len(calls) == 1 + int(flip)
            final, tags_list = inference.aggregate_results(s, final, tags_list, heatmaps, tags, scales, flip, True)
        if len(scales) != 1:
            final = inference.resize_combine(final, final.shape[2:], div=float(len(scales)))
        assert tuple(final.shape) == (1, J, H, W)
        tags = torch.cat(tags_list, dim=4)
        assert tags.shape[-1] == 1 + int(flip)
        grouped, scores = parser.parse(final, tags, adjust, refine)
    return grouped[0], scores


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("scales", [(2, 1, 0.5), (1, 2), (1, 0.5), (1,)])
def test_parse_multi_scale_equals_the_materialised_chain(nat, scales, flip):
    order = tuple(sorted(scales, reverse=True))
    outs = _scale_outputs(3, order, seed=31)
    parser = _parser()
    res = parser.parse_multi_scale([o if flip else o[:2] for o in outs], (H, W), scales, flip)
    assert len(res) == 3
    found = 0
    for n in range(3):
        _assert_same(res[n], _materialised(parser, outs, order, flip, n))
        found += len(res[n][0])
        assert len(res[n][0]) == 0 or res[n][0].shape[1:] == (J, 4 + int(flip))
    assert found >= 3


def test_parse_multi_scale_other_parser_setting(nat):
    order = (2, 1, 0.5)
    outs = _scale_outputs(2, order, seed=57)
    parser = _parser(12, 7, 3)
    res = parser.parse_multi_scale(outs, (H, W), order, True, adjust=True, refine=False)
    for n in range(2):
        _assert_same(res[n], _materialised(parser, outs, order, True, n, True, False))


IMAGE_SHAPES = [(192, 256), (256, 192), (192, 256), (192, 256), (256, 192)]     # two input-size groups, mixed


@pytest.fixture(scope="module")
def ms_batch(nat, teacher):
    from rtpe import inference
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in IMAGE_SHAPES]
    parser = _parser()
    got = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(2, 1, 0.5),
                                                flip_test=True, batch_size=2, device="cuda:0")
    return images, parser, got


def _same_final(got, want):
    (res, sc), (wres, wsc) = got, want
    assert len(res) == len(wres)
    for a, b in zip(res, wres):
        assert np.array_equal(a, b)
    assert np.array_equal(np.array(sc, np.float32), np.array(wsc, np.float32))


def test_multi_scale_batch_inference_equals_the_per_image_protocol(ms_batch, teacher):
    from rtpe import inference
    images, parser, got = ms_batch
    assert len(got) == len(images)
    people = 0
    for img, g in zip(images, got):
        want_res, want_sc, final, tags = inference.multi_scale_inference(teacher, parser, img, 256, (2, 1, 0.5), True,
                                                                         True, device="cuda:0")
        assert tags.shape[-1] == 2
        _same_final(g, (want_res, want_sc))
        people += len(want_res)
    assert people >= 1


def test_sub_batches_of_one_image_give_the_same_bits(ms_batch, teacher):
    from rtpe import inference
    images, parser, got = ms_batch
    # the largest scale-2 input (512 x 768) alone fills the budget: every scale-2 forward takes one image
    again = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(2, 1, 0.5),
                                                  flip_test=True, batch_size=2, max_forward_pixels=512 * 768,
                                                  device="cuda:0")
    for a, b in zip(again, got):
        _same_final(a, b)


def test_single_scale_equals_flip_test_inference(ms_batch, teacher):
    from rtpe import inference
    images, parser, _ = ms_batch
    a = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(1,),
                                              flip_test=True, batch_size=2, device="cuda:0")
    b = inference.flip_test_inference(teacher, parser, images, input_size=256, batch_size=2, device="cuda:0")
    for x, y in zip(a, b):
        _same_final(x, y)


def test_multi_scale_stream_equals_call(nat, teacher):
    from rtpe.engine import TeacherPipeline
    scales = (2, 1, 0.5)
    pipe = TeacherPipeline(teacher, device="cuda:0", flip_test=True, scale_factors=scales,
                           max_forward_pixels=2 * 256 * 384)
    batches = [[synth.make_images(3, int(128 * s), int(192 * s), seed=90 + k).to("cuda:0") for s in scales]
               for k in range(3)]
    want = [pipe(b) for b in batches]
    got = list(pipe.stream(iter(batches)))
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert len(g) == len(w) == 3
        for a, b in zip(g, w):
            _assert_same(a, b)


# ---- the pipeline's multi-scale kind at its smallest shapes -----------------------------------------------------------
SMALL_SCALES = (2, 1, 0.5)
SMALL_HW = (64, 128)            # the scale-1 input; the inputs are 128 x 256, 64 x 128 and 32 x 64
SMALL_BUDGET = 128 * 256        # the largest scale goes one image per forward (n0 = 1 occurs), the others whole


def _small_batches(count, seed=300):
    """``count`` batches of 2 images: one input tensor per scale, all different"""
    return [[synth.make_images(2, int(SMALL_HW[0] * s), int(SMALL_HW[1] * s), seed=seed + 10 * k + i).to("cuda:0")
             for i, s in enumerate(SMALL_SCALES)] for k in range(count)]


def _small_pipe(teacher, **kw):
    from rtpe.engine import TeacherPipeline
    return TeacherPipeline(teacher, _parser(), device="cuda:0", flip_test=True, scale_factors=SMALL_SCALES,
                           max_forward_pixels=SMALL_BUDGET, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(ags=True), dict(ags="mean"), dict(project2image=False)],
                         ids=["per_joint_tags", "ags", "ags_mean", "no_project"])
def test_pipeline_call_equals_parse_multi_scale_of_whole_batch_forwards(nat, teacher, kw):
    """``pipe(batch)`` against a reference that runs no line of rtpe/engine.py: the teacher forwarded here on every
    scale's WHOLE batch and on its mirror image, then the parser's own entry.  The pipeline cuts the largest scale into
    two forwards of one image; the forward is batch-invariant, so the bits are the same."""
    from rtpe import inference
    from rtpe.engine import forward_plan
    pipe = _small_pipe(teacher, **kw)
    batch = _small_batches(1)[0]
    assert [forward_plan(2, x.shape[2:], SMALL_BUDGET) for x in batch] == [[(0, 1), (1, 1)], [(0, 2)], [(0, 2)]]
    with torch.no_grad():
        outs = [tuple(teacher(x)) + tuple(teacher(inference.resize_combine(x, x.shape[2:], flip=True))) for x in batch]
    want = _parser().parse_multi_scale(outs, None if "project2image" in kw else SMALL_HW, SMALL_SCALES, True, **kw)
    got = pipe(batch)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        _assert_same(g, w)
    assert sum(len(p) for p, _ in want) >= 1


def test_multi_scale_stream_stopped_early_leaves_the_stream_synchronised(nat, teacher):
    pipe = _small_pipe(teacher)
    batches = _small_batches(4)
    gen = pipe.stream(iter(batches), in_flight=2, decode_stream="side")
    first = next(gen)
    gen.close()                                                     # three batches were submitted, one was taken
    again = pipe(batches[0])                                        # on the caller's stream, right behind the closed loop
    assert len(first) == len(again) == 2
    for a, b in zip(first, again):
        _assert_same(a, b)
    torch.cuda.synchronize()


def test_multi_scale_argument_errors(nat):
    from rtpe.engine import TeacherPipeline
    from rtpe.third_party.group import HeatmapParser
    outs = _scale_outputs(2, (2, 1), seed=3)
    parser = _parser()
    with pytest.raises(ValueError):
        parser.parse_multi_scale(outs[:1], (H, W), (2, 1), True)
    with pytest.raises(ValueError):
        parser.parse_multi_scale([o[:2] for o in outs], (H, W), (2, 1), True)
    with pytest.raises(ValueError):
        parser.parse_multi_scale(outs, (H, W), (2, 0.5), True)
    no_tpj = HeatmapParser(J, 30, 0.1, 1.0, True, False, tag_per_joint=False)
    with pytest.raises(ValueError):
        no_tpj.parse_multi_scale(outs, (H, W), (2, 1), True)
    with pytest.raises(ValueError):
        TeacherPipeline(torch.nn.Identity(), no_tpj, device="cuda:0", scale_factors=(2, 1))
    pipe = TeacherPipeline(torch.nn.Identity(), parser, device="cuda:0", scale_factors=(2, 1))
    with pytest.raises(ValueError):
        pipe(torch.zeros((1, 3, 64, 64), device="cuda:0"))
