"""Batched flip-test decode on the GPU (HeatmapParser.parse_flip, TeacherPipeline(flip_test=True),
inference.flip_test_inference): bit-identical, image by image, to the materialised single-scale flip test of
rtpe/inference.py (get_multi_stage_outputs + aggregate_results on the resize_combine kernel, then parser.parse),
which test_gpu_parity.py pins against the torch restatement of the upstream protocol."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import synth

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
    cache = {}

    def make(variant):
        if variant not in cache:
            sd = synth.make_state_dict(w48_shapes, 0, variant)
            cache[variant] = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to("cuda:0")
        return cache[variant]
    return make


def _parser(K=30, ksize=5, pad=2):
    from rtpe.third_party.group import HeatmapParser
    return HeatmapParser(J, K, 0.1, 1.0, True, False, nms_ksize=ksize, nms_padding=pad)


def _blob_outputs(N, H, W, seed, persons=3):
    """teacher-shaped outputs (preds (N,2J,H/4,W/4), refined (N,J,H/2,W/2)) made of structured blob maps, and those of
    the mirror images: the mirrored maps with left / right joints swapped (what a mirror-equivariant network gives),
    scaled and shifted so that the two halves of the flip average differ"""
    from rtpe.inference import FLIP_CONFIG
    perm = FLIP_CONFIG["COCO"]
    preds, refined = [], []
    for n in range(N):
        det2, _ = synth.make_decode_maps(persons, H // 2, W // 2, seed=seed + n, sigma=1.5)
        det4, tag4 = synth.make_decode_maps(persons, H // 4, W // 4, seed=seed + n, sigma=1.0)
        preds.append(np.concatenate([det4, tag4[..., 0]], axis=1))
        refined.append(det2)
    P, R = torch.from_numpy(np.concatenate(preds)), torch.from_numpy(np.concatenate(refined))
    Pf = torch.flip(P, [3])[:, perm + [J + q for q in perm]] * 0.93 + 0.004
    Rf = torch.flip(R, [3])[:, perm] * 0.91 - 0.002
    return [t.contiguous().to("cuda:0") for t in (P, R, Pf, Rf)]


def _materialised(parser, P, R, Pf, Rf, n, adjust=True, refine=True):
    """image n through the per-image flip test of rtpe/inference.py, with a stand-in model that returns the given
    outputs (the mirrored input gets the mirror image's)"""
    from rtpe import inference
    calls = []

    def model(image):
        calls.append(image)
        return [t[n:n + 1] for t in ((P, R) if len(calls) == 1 else (Pf, Rf))]
    H, W = 2 * R.shape[2], 2 * R.shape[3]
    image = torch.zeros((1, 3, H, W), device="cuda:0")
    with torch.no_grad():
        _, heatmaps, tags = inference.get_multi_stage_outputs(model, image, True, True, (W, H))
        final, tags_list = inference.aggregate_results(1, None, [], heatmaps, tags, (1,), True, True)
    assert len(calls) == 2 and tuple(final.shape) == (1, J, H, W)
    grouped, scores = parser.parse(final, torch.cat(tags_list, dim=4), adjust, refine)
    return grouped[0], scores


def _assert_same(got, want):
    (gp, gs), (wp, ws) = got, want
    assert np.array_equal(gp, wp), (gp.shape, np.asarray(wp).shape)
    assert np.array_equal(np.array(gs, np.float32), np.array(ws, np.float32))


@pytest.mark.parametrize("H,W", [(256, 256), (192, 320)])
@pytest.mark.parametrize("adjust,refine", [(True, True), (True, False), (False, True), (False, False)])
def test_parse_flip_equals_the_materialised_chain(nat, H, W, adjust, refine):
    P, R, Pf, Rf = _blob_outputs(3, H, W, seed=21)
    parser = _parser()
    res = parser.parse_flip(P, R, Pf, Rf, adjust=adjust, refine=refine)
    assert len(res) == 3
    for n in range(3):
        want = _materialised(parser, P, R, Pf, Rf, n, adjust, refine)
        _assert_same(res[n], want)
        assert len(res[n][0]) >= 1 and res[n][0].shape[1:] == (J, 5)


@pytest.mark.parametrize("K,ksize,pad", [(20, 3, 1), (12, 7, 3)])
def test_parse_flip_other_parser_settings(nat, K, ksize, pad):
    P, R, Pf, Rf = _blob_outputs(3, 192, 256, seed=40)
    parser = _parser(K, ksize, pad)
    res = parser.parse_flip(P, R, Pf, Rf, (192, 256))
    found = 0
    for n in range(3):
        _assert_same(res[n], _materialised(parser, P, R, Pf, Rf, n))
        found += len(res[n][0])
    assert found >= 3


def test_flip_test_inference_equals_the_per_image_protocol(nat, teacher):
    from rtpe import inference
    m = teacher("W0")
    rng = np.random.default_rng(3)
    shapes = [(192, 256), (256, 192), (192, 256), (192, 256), (256, 192)]          # two input-size groups, mixed
    images = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in shapes]
    parser = _parser()
    got = inference.flip_test_inference(m, parser, images, input_size=256, batch_size=2, device="cuda:0")
    assert len(got) == len(images)
    for img, (res, sc) in zip(images, got):
        want_res, want_sc, _, tags = inference.multi_scale_inference(m, parser, img, 256, (1,), True, True,
                                                                     device="cuda:0")
        assert tags.shape[-1] == 2
        assert len(res) == len(want_res)
        for a, b in zip(res, want_res):
            assert np.array_equal(a, b)
        assert np.array_equal(np.array(sc, np.float32), np.array(want_sc, np.float32))


def test_teacher_pipeline_flip_at_the_bench_size(nat, teacher):
    from rtpe.engine import TeacherPipeline
    m = teacher("W0")
    x = synth.make_images(32, 640, 640).to("cuda:0")
    parser = _parser()
    pipe = TeacherPipeline(m, parser, device="cuda:0", flip_test=True)
    res = pipe(x)
    assert len(res) == 32
    with torch.no_grad():
        P, R = m(x)
        Pf, Rf = m(torch.flip(x, [3]))
    for n in (0, 17, 31):
        _assert_same(res[n], _materialised(parser, P, R, Pf, Rf, n))


def test_flip_stream_equals_call(nat, teacher):
    from rtpe.engine import TeacherPipeline
    m = teacher("W0")
    pipe = TeacherPipeline(m, device="cuda:0", flip_test=True)
    batches = [synth.make_images(3, 128, 160, seed=70 + k).to("cuda:0") for k in range(3)]
    want = [pipe(b) for b in batches]
    got = list(pipe.stream(iter(batches)))
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert len(g) == len(w) == 3
        for a, b in zip(g, w):
            _assert_same(a, b)
    # the default pipeline is untouched by the flip one
    plain = TeacherPipeline(m, device="cuda:0")
    assert all(p.ndim != 3 or p.shape[2] == 4 for p, _ in plain(batches[0]))


def test_flip_argument_errors(nat):
    from rtpe.engine import TeacherPipeline
    from rtpe.third_party.group import HeatmapParser
    P, R, Pf, Rf = _blob_outputs(2, 128, 128, seed=5)
    parser = _parser()
    with pytest.raises(ValueError):
        parser.parse_flip(P, R, Pf, Rf, flip_index=list(range(16)))
    with pytest.raises(ValueError):
        parser.parse_flip(P, R, Pf, Rf, flip_index=[0] * J)
    with pytest.raises(ValueError):
        parser.parse_flip(P, R, Pf[:, :, :16], Rf)
    with pytest.raises(ValueError):
        parser.parse_flip(P, R[:1], Pf, Rf)
    no_tpj = HeatmapParser(J, 30, 0.1, 1.0, True, False, tag_per_joint=False)
    with pytest.raises(ValueError):
        no_tpj.parse_flip(P, R, Pf, Rf)
    with pytest.raises(ValueError):
        TeacherPipeline(torch.nn.Identity(), no_tpj, device="cuda:0", flip_test=True)
    # the native entry checks the permutation itself
    L = nat.lib()
    N, K = 2, 30
    nb = ctypes.c_size_t()
    nat.check(L.rtpe_topk_scratch_bytes(N * J, 128, 128, K, ctypes.byref(nb)))
    scratch = torch.empty(nb.value, dtype=torch.uint8, device="cuda:0")
    nat.check(L.rtpe_flip_maps_bytes(N, J, 64, 64, ctypes.byref(nb)))
    maps = torch.empty(nb.value, dtype=torch.uint8, device="cuda:0")
    val = torch.empty((N, J, K), device="cuda:0")
    ind = torch.empty((N, J, K), dtype=torch.int32, device="cuda:0")
    tag = torch.empty((N, J, K, 2), device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    def call(perm, maps_bytes):
        return L.rtpe_topk_flip(p(P), 32, 32, P.stride(0), p(R), 64, 64, R.stride(0), p(Pf), Pf.stride(0), p(Rf),
                                Rf.stride(0), N, J, (ctypes.c_int32 * J)(*perm), 128, 128, K, 5, 2, p(val), p(ind),
                                p(tag), p(maps), maps_bytes, p(scratch), scratch.numel(), nat.stream_ptr(P.device))
    with pytest.raises(RuntimeError, match="permutation"):
        nat.check(call([1] * J, maps.numel()))
    with pytest.raises(RuntimeError, match="maps buffer"):
        nat.check(call(list(range(J)), maps.numel() - 4))
    nat.check(call(list(range(J)), maps.numel()))
    torch.cuda.synchronize()
