"""Batched multi-scale / flip test WITHOUT projection to the image on the GPU (``project2image=False`` of
HeatmapParser.parse_multi_scale, TeacherPipeline, inference.multi_scale_batch_inference / flip_test_inference):
bit-identical, image by image, to the materialised per-image chain of rtpe/inference.py
``multi_scale_inference(..., project2image=False)`` - get_multi_stage_outputs + aggregate_results per scale on the
resize_combine kernel (the flip average AT each scale's refined size, the sum at the refined size r_0 of the largest
scale, the tags of scale 1 resized to r_0 unless it is first), / S, then parser.parse on the r_0 grid."""
import numpy as np
import pytest
import torch

from oracle import synth
from test_flip_decode_gpu import _assert_same, _blob_outputs, _parser
from test_multiscale_decode_gpu import IMAGE_SHAPES, _same_final, nat, teacher  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

J = 17
SIZES = [(128, 192), (160, 224)]     # scale-1 inputs; the second: grids 80 x 112 / 160 x 224, a 40 x 56 map, ratio 4
CASES = [(2, 1, 0.5), (1, 2), (1, 0.5), (1,)]
DEV = "cuda:0"


def _scale_outputs(N, H, W, scales, seed):
    """per scale (descending) the blob outputs (P, R, Pf, Rf) of a (H*s, W*s) input"""
    return [_blob_outputs(N, int(H * s), int(W * s), seed=seed + 10 * i) for i, s in enumerate(scales)]


def _materialised(parser, outs, scales, flip, n, adjust=True, refine=True):
    """image n through the per-image chain of multi_scale_inference(project2image=False), with a stand-in model per
    scale that returns the given outputs (the mirrored input gets the mirror image's)"""
    from rtpe import inference
    final, tags_list = None, []
    with torch.no_grad():
        for s, (P, R, Pf, Rf) in zip(scales, outs):
            calls = []

            def model(image):
                calls.append(image)
                return [t[n:n + 1] for t in ((P, R) if len(calls) == 1 else (Pf, Rf))]
            image = torch.zeros((1, 3, 2 * R.shape[2], 2 * R.shape[3]), device=DEV)
            _, heatmaps, tags = inference.get_multi_stage_outputs(model, image, flip, False, None)
            assert len(calls) == 1 + int(flip)
            assert all(tuple(h.shape[2:]) == tuple(R.shape[2:]) for h in heatmaps)      # nothing projected
            final, tags_list = inference.aggregate_results(s, final, tags_list, heatmaps, tags, scales, flip, False)
        if len(scales) != 1:
            final = inference.resize_combine(final, final.shape[2:], div=float(len(scales)))
        assert tuple(final.shape) == (1, J) + tuple(outs[0][1].shape[2:])               # the r_0 grid
        tags = torch.cat(tags_list, dim=4)
        assert tuple(tags.shape) == tuple(final.shape) + (1 + int(flip),)
        grouped, scores = parser.parse(final, tags, adjust, refine)
    return grouped[0], scores


_WANT = {}


def _want(H, W, order, flip, n, seed=31, N=3):
    """the materialised result of one image of the standard batch, computed once and shared"""
    key = (H, W, order, flip, n, seed, N)
    if key not in _WANT:
        _WANT[key] = _materialised(_parser(), _scale_outputs(N, H, W, order, seed), order, flip, n)
    return _WANT[key]


# ---- 1. parse level ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("scales", CASES)
@pytest.mark.parametrize("H,W", SIZES)
def test_parse_without_projection_equals_the_materialised_chain(nat, H, W, scales, flip):  # noqa: F811
    order = tuple(sorted(scales, reverse=True))
    outs = _scale_outputs(3, H, W, order, seed=31)
    parser = _parser()
    res = parser.parse_multi_scale([o if flip else o[:2] for o in outs], None, scales, flip, project2image=False)
    assert len(res) == 3
    for n in range(3):
        assert len(res[n][0]) >= 1 and res[n][0].shape[1:] == (J, 4 + int(flip))
        _assert_same(res[n], _want(H, W, order, flip, n))
    # out_hw = r_0 is the same call
    r0 = tuple(outs[0][1].shape[2:])
    again = parser.parse_multi_scale([o if flip else o[:2] for o in outs], r0, scales, flip, project2image=False)
    for a, b in zip(again, res):
        _assert_same(a, b)


# ---- 2. adjust / refine, another parser setting ----------------------------------------------------------------------
@pytest.mark.parametrize("adjust,refine", [(True, True), (True, False), (False, True), (False, False)])
def test_adjust_refine_combinations(nat, adjust, refine):  # noqa: F811
    order = (2, 1, 0.5)
    outs = _scale_outputs(2, 160, 224, order, seed=57)
    parser = _parser()
    res = parser.parse_multi_scale(outs, None, order, True, adjust=adjust, refine=refine, project2image=False)
    for n in range(2):
        assert len(res[n][0]) >= 1
        _assert_same(res[n], _materialised(parser, outs, order, True, n, adjust, refine))


def test_other_parser_setting(nat):  # noqa: F811
    order = (2, 1, 0.5)
    outs = _scale_outputs(2, 128, 192, order, seed=57)
    parser = _parser(12, 7, 3)
    res = parser.parse_multi_scale(outs, None, order, True, project2image=False)
    for n in range(2):
        assert len(res[n][0]) >= 1
        _assert_same(res[n], _materialised(parser, outs, order, True, n))


# ---- 3. sub-batches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", [(2, 1, 0.5), (1, 2)])
def test_sub_batches_of_one_image_give_the_same_bits(nat, scales):  # noqa: F811
    H, W = SIZES[1]
    order = tuple(sorted(scales, reverse=True))
    outs = _scale_outputs(3, H, W, order, seed=31)
    parser = _parser()
    hw = [tuple(o[1].shape[2:]) for o in outs]
    # scale after scale, one image at a time
    st = parser.ms_begin(3, hw, None, order, True, device=DEV, project2image=False)
    for i, o in enumerate(outs):
        for n in (2, 0, 1):
            parser.ms_prep(st, i, [t[n:n + 1] for t in o], n)
    parser.ms_topk(st)
    parser.lowres_match(st)
    by_scale = parser.lowres_finish(st)
    # image after image, every scale of one before the next one's first
    st = parser.ms_begin(3, hw, None, order, True, device=DEV, project2image=False)
    for n in range(3):
        for i, o in enumerate(outs):
            parser.ms_prep(st, i, [t[n:n + 1] for t in o], n)
    parser.ms_topk(st)
    parser.lowres_match(st)
    by_image = parser.lowres_finish(st)
    for n in range(3):
        _assert_same(by_scale[n], _want(H, W, order, True, n))
        _assert_same(by_image[n], _want(H, W, order, True, n))


def test_a_scale_before_its_predecessor_is_refused(nat):  # noqa: F811
    order = (2, 1, 0.5)
    outs = _scale_outputs(2, 128, 192, order, seed=31)
    parser = _parser()
    st = parser.ms_begin(2, [tuple(o[1].shape[2:]) for o in outs], None, order, True, device=DEV, project2image=False)
    with pytest.raises(ValueError, match="in order"):
        parser.ms_prep(st, 1, outs[1])
    parser.ms_prep(st, 0, [t[:1] for t in outs[0]], 0)
    with pytest.raises(ValueError, match="in order"):
        parser.ms_prep(st, 1, outs[1])                                  # image 1 has not passed scale 0
    with pytest.raises(ValueError, match="in order"):
        parser.ms_prep(st, 2, [t[:1] for t in outs[2]], 0)              # image 0 has not passed scale 1
    with pytest.raises(ValueError, match="once"):
        parser.ms_prep(st, 0, outs[0])                                  # image 0 would pass scale 0 twice
    parser.ms_prep(st, 1, [t[:1] for t in outs[1]], 0)
    with pytest.raises(ValueError, match="every scale"):
        parser.ms_topk(st)
    torch.cuda.synchronize()


# ---- 4. both matchers, records ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [True, False])
def test_both_matchers_agree_and_records_equal_the_list(nat, flip):  # noqa: F811
    from rtpe import engine
    from rtpe.third_party import transforms
    from rtpe.third_party.group import HeatmapParser
    H, W = SIZES[1]
    order = (2, 1, 0.5)
    outs = [o if flip else o[:2] for o in _scale_outputs(3, H, W, order, seed=31)]
    dev = HeatmapParser(J, 30, 0.1, 1.0, True, False, match_on="device")
    lists = dev.parse_multi_scale(outs, None, order, flip, project2image=False)
    for n in range(3):
        _assert_same(lists[n], _want(H, W, order, flip, n))
    h0, w0 = outs[0][1].shape[2:]
    shapes = [(300, 420), (240, 336), (301, 400)]
    meta = [transforms.get_multi_scale_size(np.zeros(s + (3,), np.uint8), 160, 0.5, 0.5)[1:] for s in shapes]
    xform = np.stack([transforms.final_preds_matrix(c, s, [w0, h0]) for c, s in meta])
    ids = [7, 581929, 0]
    rec = HeatmapParser(J, 30, 0.1, 1.0, True, False, match_on="device").parse_multi_scale(
        outs, None, order, flip, records=(ids, xform), project2image=False)
    final = [(np.stack(transforms.get_final_preds([p], c, s, [w0, h0])), sc) for (p, sc), (c, s) in zip(lists, meta)]
    want = engine.pack_records(ids, final, "cpu")
    assert rec.is_cuda and tuple(rec.shape) == tuple(want.shape)
    assert torch.equal(rec.cpu().view(torch.int32), want.view(torch.int32))


# ---- 5. end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def np_batch(nat, teacher):  # noqa: F811
    from rtpe import inference
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in IMAGE_SHAPES]
    parser = _parser()
    got = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(2, 1, 0.5),
                                                flip_test=True, batch_size=2, device=DEV, project2image=False)
    return images, parser, got


def test_batch_inference_equals_the_per_image_protocol(np_batch, teacher):  # noqa: F811
    from rtpe import inference
    images, parser, got = np_batch
    assert len(got) == len(images)
    people = 0
    for img, g in zip(images, got):
        want_res, want_sc, final, tags = inference.multi_scale_inference(teacher, parser, img, 256, (2, 1, 0.5), True,
                                                                         False, device=DEV)
        assert tags.shape[-1] == 2 and tuple(tags.shape[:4]) == tuple(final.shape)
        _same_final(g, (want_res, want_sc))
        people += len(want_res)
    assert people >= 1


def test_one_image_per_scale_2_forward_changes_no_bit(np_batch, teacher):  # noqa: F811
    from rtpe import inference
    images, parser, got = np_batch
    again = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(2, 1, 0.5),
                                                  flip_test=True, batch_size=2, max_forward_pixels=512 * 768,
                                                  device=DEV, project2image=False)
    for a, b in zip(again, got):
        _same_final(a, b)


def test_flip_test_inference_without_projection(np_batch, teacher):  # noqa: F811
    from rtpe import inference
    images, parser, _ = np_batch
    a = inference.flip_test_inference(teacher, parser, images, input_size=256, batch_size=2, device=DEV,
                                      project2image=False)
    b = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(1,),
                                              flip_test=True, batch_size=2, device=DEV, project2image=False)
    people = 0
    for x, y, img in zip(a, b, images):
        _same_final(x, y)
        want = inference.multi_scale_inference(teacher, parser, img, 256, (1,), True, False, device=DEV)
        _same_final(x, want[:2])
        people += len(want[0])
    assert people >= 1


def test_driver_records_equal_the_list_result(nat, teacher):  # noqa: F811
    """``image_ids`` of the drivers: the record kernel's ``xform`` is the ``[w2_0, h2_0]`` affine of ``get_final_preds``"""
    from rtpe import engine, inference
    rng = np.random.default_rng(4)
    images = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in ((120, 160), (150, 200), (120, 160))]
    ids = [5, 581929, 0]
    kw = dict(input_size=128, scale_factors=(1, 0.5), flip_test=True, batch_size=2, device=DEV, match_on="device",
              project2image=False)
    results = inference.multi_scale_batch_inference(teacher, _parser(), images, **kw)
    lists = [(np.stack(f) if len(f) else np.array([], np.float32), s) for f, s in results]
    want = engine.pack_records(ids, lists, "cpu")
    rec = inference.multi_scale_batch_inference(teacher, _parser(), images, image_ids=ids, **kw)
    assert rec.is_cuda and torch.equal(rec.cpu().view(torch.int32), want.view(torch.int32))
    assert sum(len(f) for f, _ in results) >= 1


# ---- 6. pipeline ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode_stream", ["side", "same"])
@pytest.mark.parametrize("in_flight", [1, 2])
def test_stream_equals_call(nat, teacher, in_flight, decode_stream):  # noqa: F811
    from rtpe.engine import TeacherPipeline
    scales = (2, 1, 0.5)
    pipe = TeacherPipeline(teacher, device=DEV, flip_test=True, scale_factors=scales,
                           max_forward_pixels=2 * 256 * 384, project2image=False)
    batches = [[synth.make_images(3, int(128 * s), int(192 * s), seed=90 + k).to(DEV) for s in scales]
               for k in range(4)]
    want = [pipe(b) for b in batches]
    got = list(pipe.stream(iter(batches), in_flight=in_flight, decode_stream=decode_stream))
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert len(g) == len(w) == 3
        for a, b in zip(g, w):
            _assert_same(a, b)
    # out_hw = r_0 is accepted, and the rows are in pixels of that grid
    _assert_same(pipe(batches[0], out_hw=(128, 192))[0], want[0][0])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_reach_no_gpu_work(nat, teacher):  # noqa: F811
    from rtpe.engine import TeacherPipeline
    outs = _scale_outputs(2, 128, 192, (2, 1), seed=3)
    parser = _parser()
    for ags in (True, "first", "mean"):
        with pytest.raises(ValueError, match="ags"):
            parser.parse_multi_scale(outs, None, (2, 1), True, ags=ags, project2image=False)
        with pytest.raises(ValueError, match="ags"):
            TeacherPipeline(teacher, _parser(), device=DEV, scale_factors=(2, 1), ags=ags, project2image=False)
    with pytest.raises(ValueError, match="decode grid"):
        parser.parse_multi_scale(outs, (256, 384), (2, 1), True, project2image=False)       # (r_0 is (128, 192))
    with pytest.raises(ValueError, match="contain 1"):
        parser.parse_multi_scale(outs, None, (2, 0.5), True, project2image=False)
    with pytest.raises(ValueError, match="at most 4"):
        parser.ms_begin(1, [(64, 64), (48, 48), (32, 32), (16, 16), (8, 8)], None, (4, 3, 2, 1, 0.5), True, device=DEV,
                        project2image=False)
    with pytest.raises(ValueError, match="scale_factors"):
        TeacherPipeline(teacher, parser, device=DEV, flip_test=True, project2image=False)
    calls = []
    pipe = TeacherPipeline(teacher, parser, device=DEV, flip_test=True, scale_factors=(2, 1), project2image=False)
    pipe.model = lambda x: calls.append(1)                  # any forward would show
    xs = [torch.zeros((1, 3, 128, 128), device=DEV), torch.zeros((1, 3, 64, 64), device=DEV)]
    with pytest.raises(ValueError, match="decode grid"):
        pipe(xs, out_hw=(128, 128))                         # (the input size; r_0 is (64, 64))
    with pytest.raises(ValueError, match="decode grid"):
        next(pipe.stream(iter([xs]), out_hw=(32, 32)))
    assert not calls
    torch.cuda.synchronize()
