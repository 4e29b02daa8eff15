"""The averaged-tag test on the GPU (``ags="mean"``, the reference's legacy/valid_ae_avg.py): ``inference.channel_mean``
against PyTorch-CPU's ``mean(dim=1)`` bit for bit; ``HeatmapParser.parse_multi_scale(ags="mean")`` against the
materialised per-image chain whose tag map is ``tags[0].cpu().mean(dim=1)`` - the CPU op is the yardstick, not the
kernel; and the batched drivers, the pipeline and the device-resident records against the per-image
``multi_scale_inference(ags="mean")`` with the W0 teacher."""
import numpy as np
import pytest
import torch

from oracle import synth
from test_ags_decode_gpu import IMAGE_SHAPES
from test_flip_decode_gpu import _assert_same, _blob_outputs, _parser
from test_multiscale_decode_gpu import H, W, _same_final
from test_tag_mean_host import mean_restated, seeded

pytestmark = pytest.mark.gpu

J = 17
DEV = "cuda:0"


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
    return build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the op ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 17, 1, 32), (2, 17, 4, 24), (1, 16, 8, 8), (1, 18, 8, 8), (1, 32, 4, 16),
                                   (1, 1, 2, 16), (1, 272, 2, 16)])
def test_channel_mean_equals_torch_cpu(nat, shape):
    """every plane here has a multiple of 32 pixels: ATen's vectorised order everywhere"""
    from rtpe import inference
    x = seeded(shape, 21)
    got = inference.channel_mean(x.to(DEV))
    assert tuple(got.shape) == (shape[0],) + shape[2:] and got.dtype == torch.float32 and got.is_cuda
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(x.mean(dim=1).numpy()))


def test_channel_mean_of_a_channel_slice(nat):
    """``t[:, 17:]`` of a (2,34,8,12) tensor is read where it is (the strides go to the kernel)"""
    from rtpe import inference
    t = seeded((2, 34, 8, 12), 22)
    d = t.to(DEV)
    for sl in (slice(17, None), slice(0, 17), slice(3, 21)):
        got = inference.channel_mean(d[:, sl])
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(t[:, sl].mean(dim=1).numpy())), sl
    got = inference.channel_mean(d[1:, 17:])                                  # (a batch slice on top)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(t[1:, 17:].mean(dim=1).numpy()))
    assert torch.equal(d.cpu(), t)                                            # (the input is only read)


def test_channel_mean_tail_pixels_follow_the_pinned_order(nat):
    """(1,17,7,33): the restatement for all 231 pixels, torch below 224 = 231 // 32 * 32 (beyond it ATen takes another
    order, tests/test_tag_mean_host.py)"""
    from rtpe import inference
    x = seeded((1, 17, 7, 33), 12)
    got = inference.channel_mean(x.to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(mean_restated(x.numpy())))
    assert np.array_equal(_bits(got.reshape(-1)[:224]), _bits(x.mean(dim=1).numpy().reshape(-1)[:224]))


def test_channel_mean_of_negative_zeros_is_plus_zero(nat):
    from rtpe import inference
    x = seeded((2, 17, 4, 16), 23)
    x[1] = -0.0
    got = inference.channel_mean(x.to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(x.mean(dim=1).numpy()))
    assert (got[1] == 0).all() and not np.signbit(got[1]).any()


def test_channel_mean_argument_errors(nat):
    from rtpe import inference
    with pytest.raises(TypeError):
        inference.channel_mean(torch.zeros((1, 17, 4, 8), dtype=torch.float16, device=DEV))
    with pytest.raises(TypeError):
        inference.channel_mean(torch.zeros((17, 4, 8), device=DEV))
    with pytest.raises(ValueError):
        inference.channel_mean(torch.zeros((1, 0, 4, 8), device=DEV))
    with pytest.raises(ValueError, match="272"):            # (the CPU op's order is pinned up to 272 channels)
        inference.channel_mean(torch.zeros((1, 273, 2, 16), device=DEV))


# ---- the decode against the materialised chain ---------------------------------------------------------------------------
def _mean_outputs(N, scales, seed):
    """per scale (descending) the blob outputs (P, R, Pf, Rf) of a (H*s, W*s) input, the same people at every scale.
    EVERY tag channel carries the person's tag on all joints' blobs (the maximum over the joints' tag maps, as
    test_ags_decode_gpu._ags_outputs makes channel J) plus a seeded 0.01 * randn of its own: the mean over the channels
    is a usable shared tag, and it is not any single channel"""
    outs = [_blob_outputs(N, int(H * s), int(W * s), seed=seed) for s in scales]
    g = torch.Generator().manual_seed(seed)
    for o in outs:
        for P in (o[0], o[2]):
            noise = 0.01 * torch.randn(P[:, J:].shape, generator=g)
            P[:, J:] = P[:, J:].amax(1, keepdim=True) + noise.to(P.device)
    return outs


def _materialised_mean(parser, outs, scales, flip, n, adjust=True, refine=True):
    """image n through the per-image chain (get_multi_stage_outputs + aggregate_results + the / S) with a stand-in
    model per scale; the tag map is PyTorch-CPU's ``mean(dim=1)`` of the first tag tensor of the LAST scale, moved back"""
    from rtpe import inference
    final, tags_list, last = None, [], None
    with torch.no_grad():
        for s, (P, R, Pf, Rf) in zip(scales, outs):
            calls = []

            def model(image):
                calls.append(image)
                return [t[n:n + 1] for t in ((P, R) if len(calls) == 1 else (Pf, Rf))]
            image = torch.zeros((1, 3, 2 * R.shape[2], 2 * R.shape[3]), device=DEV)
            _, heatmaps, tags = inference.get_multi_stage_outputs(model, image, flip, True, (W, H))
            assert len(calls) == 1 + int(flip)
            last = tags[0]
            final, tags_list = inference.aggregate_results(s, final, tags_list, heatmaps, tags, scales, flip, True)
        if len(scales) != 1:
            final = inference.resize_combine(final, final.shape[2:], div=float(len(scales)))
        assert tuple(final.shape) == (1, J, H, W) and tuple(last.shape) == (1, J, H, W) and (H * W) % 32 == 0
        mean = last.cpu().mean(dim=1).to(DEV)                      # the yardstick: the CPU op
        assert not parser.tag_per_joint
        grouped, scores = parser.parse(final, mean.unsqueeze(-1).unsqueeze(0).contiguous(), adjust, refine)
    return grouped[0], scores


def _shared_parser(K=30, ksize=5, pad=2):
    p = _parser(K, ksize, pad)
    p.tag_per_joint = False
    return p


def _check_batch(res, outs, order, flip, parser_args=(), adjust=True, refine=True):
    """every image of the batch against the chain -> (people, people with 3 or more detected joints)"""
    ref = _shared_parser(*parser_args)
    found, multi = 0, 0
    for n in range(len(res)):
        _assert_same(res[n], _materialised_mean(ref, outs, order, flip, n, adjust, refine))
        people = res[n][0]
        found += len(people)
        if len(people):
            assert people.shape[1:] == (J, 4)
            multi += int(((people[:, :, 2] > 0).sum(1) >= 3).sum())
    return found, multi


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("scales", [(2, 1, 0.5), (1, 2), (1, 0.5), (1,)])
def test_parse_multi_scale_mean_equals_the_materialised_chain(nat, scales, flip):
    order = tuple(sorted(scales, reverse=True))
    outs = _mean_outputs(3, order, seed=31)
    given = [o if flip else o[:2] for o in outs]
    parser = _parser()                                  # tag_per_joint=True: not consulted with ags="mean"
    res = parser.parse_multi_scale(given, (H, W), scales, flip, ags="mean")
    assert len(res) == 3 and parser.tag_per_joint
    found, _ = _check_batch(res, outs, order, flip)
    assert found >= 3
    # the mean matters: on the same outputs the first channel gives another result in at least one image
    first = parser.parse_multi_scale(given, (H, W), scales, flip, ags=True)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(res, first))
    again = parser.parse_multi_scale(given, (H, W), scales, flip, ags="first")
    for a, b in zip(first, again):
        _assert_same(a, b)


@pytest.mark.parametrize("adjust,refine", [(True, True), (True, False), (False, True), (False, False)])
def test_parse_multi_scale_mean_adjust_refine(nat, adjust, refine):
    order = (2, 1, 0.5)
    outs = _mean_outputs(3, order, seed=43)
    res = _shared_parser().parse_multi_scale(outs, (H, W), order, True, adjust=adjust, refine=refine, ags="mean")
    found, multi = _check_batch(res, outs, order, True, adjust=adjust, refine=refine)
    assert found >= 3
    if not refine:
        assert multi >= 3, "the averaged tag should group several detected joints per person"


def test_parse_multi_scale_mean_other_parser_setting(nat):
    order = (2, 1, 0.5)
    outs = _mean_outputs(3, order, seed=57)
    res = _shared_parser(12, 7, 3).parse_multi_scale(outs, (H, W), order, True, adjust=True, refine=False, ags="mean")
    found, multi = _check_batch(res, outs, order, True, (12, 7, 3), True, False)
    assert found >= 3 and multi >= 3


def test_mean_planes_written_per_sub_batch(nat):
    """the phases with one image per ms_prep at every scale, out of order: the same bits as the whole batch, which is
    checked against the chain"""
    order = (2, 1, 0.5)
    outs = _mean_outputs(3, order, seed=71)
    parser = _parser()
    want = parser.parse_multi_scale(outs, (H, W), order, True, ags="mean")
    found, _ = _check_batch(want, outs, order, True)
    assert found >= 3
    st = parser.ms_begin(3, [tuple(o[1].shape[2:]) for o in outs], (H, W), order, True, device=DEV, ags="mean")
    for i, o in enumerate(outs):
        for n0 in (2, 0, 1):
            parser.ms_prep(st, i, [t[n0:n0 + 1] for t in o], n0)
    parser.ms_topk(st)
    parser.lowres_match(st)
    got = parser.lowres_finish(st)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        _assert_same(a, b)


def test_mean_device_grouping_and_records(nat):
    """``match_on="device"``: the same rows; with records, ``pack_records`` of them"""
    from rtpe import engine
    from test_records_gpu import _equal, _host_records, _xform
    order = (2, 1, 0.5)
    outs = _mean_outputs(3, order, seed=31)
    want = _parser().parse_multi_scale(outs, (H, W), order, True, ags="mean")
    dev = _parser()
    dev.match_on = "device"
    got = dev.parse_multi_scale(outs, (H, W), order, True, ags="mean")
    for a, b in zip(got, want):
        _assert_same(a, b)
    ids, xf = [7, 1 << 24, 0], _xform(3)
    rec = dev.parse_multi_scale(outs, (H, W), order, True, ags="mean", records=(ids, xf))
    assert tuple(rec.shape) == (3, engine.RECORD_FLOATS)
    _equal(rec, _host_records(ids, want, xf))
    assert sum(len(p) for p, _ in want) >= 3


# ---- end to end with the W0 teacher ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mean_batch(nat, teacher):
    from rtpe import inference
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in IMAGE_SHAPES]
    parser = _parser()
    got = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(2, 1, 0.5),
                                                flip_test=True, batch_size=2, device=DEV, ags="mean")
    return images, parser, got


@pytest.fixture(scope="module")
def per_image(nat, teacher, mean_batch):
    """the per-image protocol, computed once: ``{scales: [(final_results, scores)]}``"""
    from rtpe import inference
    images = mean_batch[0]
    out = {}
    for scales in ((2, 1, 0.5), (1,)):
        rows = []
        for img in images:
            res, sc, final, tags = inference.multi_scale_inference(teacher, _parser(), img, 256, scales, True, True,
                                                                   device=DEV, ags="mean")
            assert tuple(tags.shape) == (1, 1) + tuple(final.shape[2:]) + (1,)
            assert (final.shape[2] * final.shape[3]) % 32 == 0
            rows.append((res, sc))
        out[scales] = rows
    return out


def test_multi_scale_batch_inference_mean_equals_the_per_image_protocol(mean_batch, per_image):
    images, parser, got = mean_batch
    assert parser.tag_per_joint is False                # set and left set, as the per-image call does
    assert len(got) == len(images)
    for g, want in zip(got, per_image[(2, 1, 0.5)]):
        _same_final(g, want)
    assert sum(len(r) for r, _ in per_image[(2, 1, 0.5)]) >= 1


def test_per_image_mean_is_the_cpu_mean_of_its_tag_maps(nat, teacher, mean_batch):
    """the per-image chain's tag map against the CPU op on the maps it was made of"""
    from rtpe import inference
    from rtpe.third_party import transforms
    img = mean_batch[0][0]
    p = _parser()
    _, _, final, tags = inference.multi_scale_inference(teacher, p, img, 256, (1,), True, True, device=DEV, ags="mean")
    assert p.tag_per_joint is False
    base, _, _ = transforms.get_multi_scale_size(img, 256, 1.0, 1)
    with torch.no_grad():
        t, _, _ = transforms.warp_normalize(img, 256, 1, 1, device=DEV)
        _, _, maps = inference.get_multi_stage_outputs(teacher, t, True, True, base)
    want = maps[0].cpu().mean(dim=1)
    assert np.array_equal(_bits(tags[0, 0, :, :, 0].cpu().numpy()), _bits(want[0].numpy()))
    assert not torch.equal(tags[0, 0, :, :, 0].cpu(), maps[0][0, 0].cpu())


def test_mean_sub_batches_of_one_image_give_the_same_bits(mean_batch, teacher):
    from rtpe import inference
    images, parser, got = mean_batch
    # the largest scale-2 input (512 x 768) alone fills the budget: every scale-2 forward takes one image
    again = inference.multi_scale_batch_inference(teacher, parser, images, input_size=256, scale_factors=(2, 1, 0.5),
                                                  flip_test=True, batch_size=2, max_forward_pixels=512 * 768,
                                                  device=DEV, ags="mean")
    assert len(again) == len(got)
    for a, b in zip(again, got):
        _same_final(a, b)


def test_flip_test_inference_mean_equals_the_per_image_protocol(mean_batch, per_image, teacher):
    from rtpe import inference
    images = mean_batch[0]
    parser = _parser()
    got = inference.flip_test_inference(teacher, parser, images, input_size=256, batch_size=2, device=DEV, ags="mean")
    assert parser.tag_per_joint is False
    # the scale-1 inputs are 256 x 384 / 384 x 256: one image per forward, the tag maps and planes written per image
    one = inference.multi_scale_batch_inference(teacher, _parser(), images, input_size=256, scale_factors=(1,),
                                                flip_test=True, batch_size=2, max_forward_pixels=256 * 384,
                                                device=DEV, ags="mean")
    assert len(got) == len(one) == len(images)
    for g, o, want in zip(got, one, per_image[(1,)]):
        _same_final(g, want)
        _same_final(o, want)
    assert sum(len(r) for r, _ in per_image[(1,)]) >= 1


def test_mean_stream_equals_call(nat, teacher):
    from rtpe.engine import TeacherPipeline
    scales = (2, 1, 0.5)
    pipe = TeacherPipeline(teacher, device=DEV, flip_test=True, scale_factors=scales,
                           max_forward_pixels=2 * 256 * 384, ags="mean")
    assert pipe.ags == "mean"
    batches = [[synth.make_images(3, int(128 * s), int(192 * s), seed=90 + k).to(DEV) for s in scales]
               for k in range(3)]
    want = [pipe(b) for b in batches]
    got = list(pipe.stream(iter(batches)))
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert len(g) == len(w) == 3
        for a, b in zip(g, w):
            _assert_same(a, b)
            assert len(a[0]) == 0 or a[0].shape[1:] == (J, 4)


def test_mean_driver_records(mean_batch, teacher):
    """``match_on="device"`` with ``image_ids``: the record tensor is ``pack_records`` of the list result"""
    from rtpe import inference
    from test_records_gpu import _driver_records, _equal
    images, _, got = mean_batch
    ids = [5, 581929, 0, 1 << 24, 42]
    kw = dict(input_size=256, scale_factors=(2, 1, 0.5), flip_test=True, batch_size=2, device=DEV, ags="mean",
              match_on="device")
    lists = inference.multi_scale_batch_inference(teacher, _parser(), images, **kw)
    for a, b in zip(lists, got):                        # device grouping: the bits of host grouping
        _same_final(a, b)
    want, people = _driver_records(ids, lists)
    _equal(inference.multi_scale_batch_inference(teacher, _parser(), images, image_ids=ids, **kw), want)
    assert people >= 1
