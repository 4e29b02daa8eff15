"""Batched AGS multi-scale test on the GPU (HeatmapParser.parse_multi_scale(ags=True), TeacherPipeline(ags=True),
inference.multi_scale_batch_inference / flip_test_inference(ags=True)): bit-identical, image by image, to the AGS
branch of rtpe/inference.py multi_scale_inference - ONE tag map for all joints, channel 0 of the un-mirrored tag
maps of the smallest scale, grouped by a parser with tag_per_joint=False - which test_gpu_parity.py pins against the
oracle."""
import numpy as np
import pytest
import torch

from oracle import synth
from test_flip_decode_gpu import _assert_same, _blob_outputs, _parser
from test_multiscale_decode_gpu import H, W, _same_final, _scale_outputs

pytestmark = pytest.mark.gpu

J = 17


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


def _ags_parser(K=30, ksize=5, pad=2):
    p = _parser(K, ksize, pad)
    p.tag_per_joint = False
    return p


def _ags_outputs(N, scales, seed):
    """per scale (descending) the blob outputs (P, R, Pf, Rf) of a (H*s, W*s) input, the same people at every scale,
    with channel J (joint 0's tag) replaced by the maximum over the joints' tag maps: every joint's blob carries its
    person's tag there (as the ags_p4 goldens)"""
    outs = [_blob_outputs(N, int(H * s), int(W * s), seed=seed) for s in scales]
    for o in outs:
        for P in (o[0], o[2]):
            P[:, J] = P[:, J:].amax(1)
    return outs


def _materialised_ags(parser, outs, scales, flip, n, adjust=True, refine=True):
    """image n through the per-image chain of multi_scale_inference(..., ags=True) with a stand-in model per scale:
    the heat maps as in the multi-scale test, the tag map = channel 0 of the first tag map of the LAST scale"""
    from rtpe import inference
    final, tags_list, ags = None, [], None
    with torch.no_grad():
        for s, (P, R, Pf, Rf) in zip(scales, outs):
            calls = []

            def model(image):
                calls.append(image)
                return [t[n:n + 1] for t in ((P, R) if len(calls) == 1 else (Pf, Rf))]
            image = torch.zeros((1, 3, 2 * R.shape[2], 2 * R.shape[3]), device="cuda:0")
            _, heatmaps, tags = inference.get_multi_stage_outputs(model, image, flip, True, (W, H))
            assert len(calls) == 1 + int(flip)
            ags = tags[0][:, 0]
            final, tags_list = inference.aggregate_results(s, final, tags_list, heatmaps, tags, scales, flip, True)
        if len(scales) != 1:
            final = inference.resize_combine(final, final.shape[2:], div=float(len(scales)))
        assert tuple(final.shape) == (1, J, H, W) and tuple(ags.shape) == (1, H, W)
        assert not parser.tag_per_joint
        grouped, scores = parser.parse(final, ags.unsqueeze(-1).unsqueeze(0).contiguous(), adjust, refine)
    return grouped[0], scores


def _check_batch(res, outs, order, flip, parser_args=(), adjust=True, refine=True):
    ref = _ags_parser(*parser_args)
    found, multi = 0, 0
    for n in range(len(res)):
        _assert_same(res[n], _materialised_ags(ref, outs, order, flip, n, adjust, refine))
        people = res[n][0]
        found += len(people)
        if len(people):
            assert people.shape[1:] == (J, 4)
            multi += int(((people[:, :, 2] > 0).sum(1) >= 3).sum())
    return found, multi


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("scales", [(2, 1, 0.5), (1, 2), (1, 0.5), (1,)])
def test_parse_multi_scale_ags_equals_the_materialised_chain(nat, scales, flip):
    order = tuple(sorted(scales, reverse=True))
    outs = _ags_outputs(3, order, seed=31)
    parser = _parser()                                  # tag_per_joint=True: not consulted with ags=True
    res = parser.parse_multi_scale([o if flip else o[:2] for o in outs], (H, W), scales, flip, ags=True)
    assert len(res) == 3 and parser.tag_per_joint
    found, _ = _check_batch(res, outs, order, flip)
    assert found >= 3


@pytest.mark.parametrize("adjust,refine", [(True, False), (False, True), (False, False)])
def test_parse_multi_scale_ags_adjust_refine(nat, adjust, refine):
    order = (2, 1, 0.5)
    outs = _ags_outputs(3, order, seed=43)
    res = _ags_parser().parse_multi_scale(outs, (H, W), order, True, adjust=adjust, refine=refine, ags=True)
    found, multi = _check_batch(res, outs, order, True, adjust=adjust, refine=refine)
    assert found >= 3
    if not refine:
        assert multi >= 3, "the shared tag should group several detected joints per person"


def test_parse_multi_scale_ags_other_parser_setting(nat):
    order = (2, 1, 0.5)
    outs = _ags_outputs(2, order, seed=57)
    res = _ags_parser(12, 7, 3).parse_multi_scale(outs, (H, W), order, True, adjust=True, refine=False, ags=True)
    _check_batch(res, outs, order, True, (12, 7, 3), True, False)


def test_ags_planes_written_per_sub_batch(nat):
    """the phases with one image per ms_prep at every scale, out of order: the same bits as the whole batch"""
    order = (2, 1, 0.5)
    outs = _ags_outputs(3, order, seed=71)
    parser = _parser()
    want = parser.parse_multi_scale(outs, (H, W), order, True, ags=True)
    st = parser.ms_begin(3, [tuple(o[1].shape[2:]) for o in outs], (H, W), order, True, device="cuda:0", ags=True)
    for i, o in enumerate(outs):
        for n0 in (2, 0, 1):
            parser.ms_prep(st, i, [t[n0:n0 + 1] for t in o], n0)
    parser.ms_topk(st)
    parser.lowres_match(st)
    got = parser.lowres_finish(st)
    for a, b in zip(got, want):
        _assert_same(a, b)


IMAGE_SHAPES = [(192, 256), (256, 192), (192, 256), (192, 256), (256, 192)]     # two input-size groups, mixed


@pytest.fixture(scope="module")
def ags_batch(nat, teacher):
    from rtpe import inference
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in IMAGE_SHAPES]
    parser = _parser()
    got = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(2, 1, 0.5),
                                                flip_test=True, batch_size=2, device="cuda:0", ags=True)
    return images, parser, got


def test_multi_scale_batch_inference_ags_equals_the_per_image_protocol(ags_batch, teacher):
    from rtpe import inference
    images, parser, got = ags_batch
    assert parser.tag_per_joint is False                # set and left set, as the per-image call does
    assert len(got) == len(images)
    people = 0
    for img, g in zip(images, got):
        want_res, want_sc, final, tags = inference.multi_scale_inference(teacher, _parser(), img, 256, (2, 1, 0.5),
                                                                         True, True, device="cuda:0", ags=True)
        assert tuple(tags.shape) == (1, 1) + tuple(final.shape[2:]) + (1,)
        _same_final(g, (want_res, want_sc))
        people += len(want_res)
    assert people >= 1


def test_ags_sub_batches_of_one_image_give_the_same_bits(ags_batch, teacher):
    from rtpe import inference
    images, parser, got = ags_batch
    # the largest scale-2 input (512 x 768) alone fills the budget: every scale-2 forward takes one image.  (No budget
    # that admits a scale-2 image splits the scale-0.5 batches; test_ags_planes_written_per_sub_batch and the
    # single-scale run below write the shared tag planes one image at a time.)
    again = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(2, 1, 0.5),
                                                  flip_test=True, batch_size=2, max_forward_pixels=512 * 768,
                                                  device="cuda:0", ags=True)
    for a, b in zip(again, got):
        _same_final(a, b)


def test_flip_test_inference_ags_equals_the_per_image_protocol(ags_batch, teacher):
    from rtpe import inference
    images, _, _ = ags_batch
    parser = _parser()
    got = inference.flip_test_inference(teacher, parser, images, input_size=256, batch_size=2, device="cuda:0",
                                        ags=True)
    assert parser.tag_per_joint is False
    # the scale-1 inputs are 256 x 384 / 384 x 256: one image per forward, the shared tag plane written per image
    one = inference.multi_scale_batch_inference(teacher, _parser(), images, input_size=256, scale_factors=(1,),
                                                flip_test=True, batch_size=2, max_forward_pixels=256 * 384,
                                                device="cuda:0", ags=True)
    people = 0
    for img, g, o in zip(images, got, one):
        want_res, want_sc, _, _ = inference.multi_scale_inference(teacher, _parser(), img, 256, (1,), True, True,
                                                                  device="cuda:0", ags=True)
        _same_final(g, (want_res, want_sc))
        _same_final(o, (want_res, want_sc))
        people += len(want_res)
    assert people >= 1


def test_ags_stream_equals_call(nat, teacher):
    from rtpe.engine import TeacherPipeline
    scales = (2, 1, 0.5)
    pipe = TeacherPipeline(teacher, device="cuda:0", flip_test=True, scale_factors=scales,
                           max_forward_pixels=2 * 256 * 384, ags=True)
    batches = [[synth.make_images(3, int(128 * s), int(192 * s), seed=90 + k).to("cuda:0") for s in scales]
               for k in range(3)]
    want = [pipe(b) for b in batches]
    got = list(pipe.stream(iter(batches)))
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert len(g) == len(w) == 3
        for a, b in zip(g, w):
            _assert_same(a, b)
            assert len(a[0]) == 0 or a[0].shape[1:] == (J, 4)


def test_ags_argument_errors(nat):
    from rtpe import inference
    from rtpe.engine import TeacherPipeline
    from rtpe.third_party.group import HeatmapParser
    for kw in (dict(), dict(flip_test=True)):
        with pytest.raises(ValueError, match="scale_factors"):
            TeacherPipeline(torch.nn.Identity(), _parser(), device="cuda:0", ags=True, **kw)
    outs = _scale_outputs(2, (2, 1), seed=3)
    no_tpj = HeatmapParser(J, 30, 0.1, 1.0, True, False, tag_per_joint=False)
    # without ags, a parser without per-joint tags is still refused by every batched entry
    with pytest.raises(ValueError):
        no_tpj.parse_multi_scale(outs, (H, W), (2, 1), True)
    with pytest.raises(ValueError):
        no_tpj.ms_begin(2, [tuple(o[1].shape[2:]) for o in outs], (H, W), (2, 1), True, device="cuda:0")
    with pytest.raises(ValueError):
        TeacherPipeline(torch.nn.Identity(), no_tpj, device="cuda:0", scale_factors=(2, 1))
    with pytest.raises(ValueError):
        TeacherPipeline(torch.nn.Identity(), no_tpj, device="cuda:0", flip_test=True)
    img = np.zeros((192, 256, 3), np.uint8)
    with pytest.raises(ValueError):
        inference.multi_scale_batch_inference(torch.nn.Identity(), no_tpj, [img], 256, (2, 1, 0.5), device="cuda:0")
    with pytest.raises(ValueError):
        inference.flip_test_inference(torch.nn.Identity(), no_tpj, [img], 256, device="cuda:0")
    assert no_tpj.tag_per_joint is False
    # with ags, it is accepted, and decodes as a parser with per-joint tags does
    TeacherPipeline(torch.nn.Identity(), no_tpj, device="cuda:0", flip_test=True, scale_factors=(2, 1), ags=True)
    a = no_tpj.parse_multi_scale(outs, (H, W), (2, 1), True, ags=True)
    b = _parser().parse_multi_scale(outs, (H, W), (2, 1), True, ags=True)
    for x, y in zip(a, b):
        _assert_same(x, y)
