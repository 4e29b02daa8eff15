"""Per-image decode size on the GPU: every image of a batch decoded at its own (h, w) (``parse_lowres`` /
``TeacherPipeline`` with a list of sizes, ``rtpe.inference.plain_inference``).  The yardstick is never the new path: it
is the oracle (``oracle.decode_ref``, pinned bit-exactly on the reference's fixtures by tests/test_oracle_golden.py), a
fixture made by the reference itself, and the existing one-size entry called for the image alone.  Every comparison is
``np.array_equal``, no image of any batch is left out of one, and every test states how many people it expects per
image, so that equal empty results cannot pass for it."""
import os

import numpy as np
import pytest
import torch

from oracle import decode_ref, synth

pytestmark = pytest.mark.gpu

J = 17
DEV = "cuda:0"
COMBOS = [(True, True), (True, False), (False, True), (False, False)]
# one batch of 8 network outputs of a 256 x 320 input (refined 128 x 160, tags 64 x 80), each decoded at its own size:
# twice the maps, between, equal to the refined maps (the samplers' copy path on both axes), odd, equal to the tag
# maps (below the refined maps), narrower than one 32 x 64 tile, portrait, and far above
MIX_P = [3, 0, 5, 2, 4, 1, 3, 6]
MIX_HW = [(256, 320), (192, 240), (128, 160), (100, 333), (64, 80), (31, 47), (300, 70), (427, 640)]


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


def _parser(match_on="host", K=30, ksize=5, pad=2):
    from rtpe.third_party.group import HeatmapParser
    return HeatmapParser(J, K, 0.1, 1.0, True, False, True, ksize, pad, match_on=match_on)


def _n_people(people):
    return len(people) if getattr(people, "ndim", 0) == 3 else 0


def _same(got, want):
    """one image: the people rows and the scores, bit for bit"""
    gp, gs = got
    wp, ws = want
    assert _n_people(gp) == _n_people(wp)
    assert np.array_equal(np.asarray(gp, np.float32), np.asarray(wp, np.float32))
    assert np.array_equal(np.array(gs, np.float32), np.array(ws, np.float32))


def _mix_batch():
    sets = [synth.make_lowres_maps(p, 256, 320, seed=50 + i) for i, p in enumerate(MIX_P)]
    refined = torch.from_numpy(np.concatenate([s[0] for s in sets]))
    tags = torch.from_numpy(np.concatenate([s[1] for s in sets]))
    assert tuple(refined.shape) == (8, J, 128, 160) and tuple(tags.shape) == (8, J, 64, 80)
    return refined, tags


def _oracle(refined, tags, n, hw, adjust=True, refine=True, ref=None):
    """image n at hw: F.interpolate(align_corners=True) of both maps + parse (validate_hhrnet.py:93-101)"""
    ref = ref or decode_ref.HeatmapParserRef()
    hms = decode_ref.upsample_bilinear(refined[n:n + 1], hw[0], hw[1])
    aes = decode_ref.upsample_bilinear(tags[n:n + 1], hw[0], hw[1])
    ans, scores = ref.parse(hms, aes.unsqueeze(-1), adjust, refine)
    return ans[0], scores


def _one_by_one(parser, refined, tags, sizes, adjust=True, refine=True):
    """the existing one-size entry, one image at a time"""
    return [parser.parse_lowres(refined[n:n + 1], tags[n:n + 1], tuple(hw), adjust, refine)[0]
            for n, hw in enumerate(sizes)]


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("adjust,refine", COMBOS)
def test_mixed_batch_equals_the_oracle_at_every_images_own_size(nat, adjust, refine, match_on):
    refined, tags = _mix_batch()
    got = _parser(match_on).parse_lowres(refined.to(DEV), tags.to(DEV), MIX_HW, adjust, refine)
    assert len(got) == 8
    for n, (hw, p) in enumerate(zip(MIX_HW, MIX_P)):
        want = _oracle(refined, tags, n, hw, adjust, refine)
        assert _n_people(want[0]) == p, (n, hw)
        _same(got[n], want)
        if p:
            assert got[n][0].shape == (p, J, 4) and got[n][0].dtype == np.float32
            assert got[n][0][:, :, 0].max() < hw[1] + 1 and got[n][0][:, :, 1].max() < hw[0] + 1   # its own pixels
            if refine:
                assert (got[n][0][:, :, 2] > 0).all()                   # every joint filled
    assert sum(MIX_P) == 24


# outputs around the size at which PyTorch's CPU op changes its kernel (oh + ow <= 128: the weights are multiplied first
# and four products summed, the 17th channel in a scalar loop): 128 and 129, flat, narrow, one pixel wide
SMALL_HW = [(64, 64), (128, 1), (20, 100), (48, 48), (100, 28), (29, 99), (40, 88), (64, 65)]
SMALL_P = [3, 0, 7, 2, 4, 1, 3, 6]            # what the oracle finds there (image 2 is squashed 6 : 1)


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_small_outputs_follow_the_other_kernel_of_the_cpu_op(nat, match_on):
    """every image against the oracle, in one batch with per-image sizes AND alone through the one-size entry"""
    refined, tags = _mix_batch()
    r, t = refined.to(DEV), tags.to(DEV)
    got = _parser(match_on).parse_lowres(r, t, SMALL_HW)
    alone = _one_by_one(_parser(match_on), r, t, SMALL_HW)
    for n, (hw, p) in enumerate(zip(SMALL_HW, SMALL_P)):
        want = _oracle(refined, tags, n, hw)
        assert _n_people(want[0]) == p, (n, hw)
        _same(got[n], want)
        _same(alone[n], want)


def test_mixed_batch_device_grouping_equals_host_grouping(nat):
    refined, tags = _mix_batch()
    r, t = refined.to(DEV), tags.to(DEV)
    for adjust, refine in COMBOS:
        host = _parser("host").parse_lowres(r, t, MIX_HW, adjust, refine)
        dev = _parser("device").parse_lowres(r, t, MIX_HW, adjust, refine)
        for n in range(8):
            _same(dev[n], host[n])
            assert _n_people(host[n][0]) == MIX_P[n]


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("K,ksize,pad", [(20, 3, 1), (12, 7, 3)])
def test_mixed_batch_other_windows_equal_the_one_size_entry(nat, K, ksize, pad, match_on):
    """other people caps and NMS windows: the run-time-padding instantiation of the tile kernel"""
    refined, tags = _mix_batch()
    r, t = refined.to(DEV), tags.to(DEV)
    got = _parser(match_on, K, ksize, pad).parse_lowres(r, t, MIX_HW)
    want = _one_by_one(_parser("host", K, ksize, pad), r, t, MIX_HW)
    ref = decode_ref.HeatmapParserRef(J, K, 0.1, 1.0, True, False, True, ksize, pad)
    for n in range(8):
        _same(got[n], want[n])
        _same(got[n], _oracle(refined, tags, n, MIX_HW[n], ref=ref))
        assert _n_people(got[n][0]) == MIX_P[n]


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("place", [0, 1, 3])
def test_reference_fixture_inside_a_mixed_batch(nat, golden_dir, place, match_on):
    """decode_lowres_p2_nonsq.npz - made by the reference: a 640 x 896 network input decoded at 427 x 640 - first, in the
    middle and last among maps of the same input size decoded at 480 x 640, 375 x 500 and 640 x 896"""
    g = np.load(os.path.join(golden_dir, "decode_lowres_p2_nonsq.npz"))
    P, H, W, oh, ow, seed = [int(v) for v in g["meta"]]
    assert (P, H, W, oh, ow) == (2, 640, 896, 427, 640)
    others = [(3, 81, (480, 640)), (4, 82, (375, 500)), (2, 83, (640, 896))]
    items = [(synth.make_lowres_maps(p, 640, 896, seed=s), hw, p) for p, s, hw in others]
    items.insert(place, (synth.make_lowres_maps(P, H, W, seed=seed), (oh, ow), P))
    refined = torch.from_numpy(np.concatenate([it[0][0] for it in items])).to(DEV)
    tags = torch.from_numpy(np.concatenate([it[0][1] for it in items]))
    preds = torch.zeros((4, 2 * J) + tuple(tags.shape[2:]))            # the tags as the channel slice forward() returns
    preds[:, J:] = tags
    tags = preds.to(DEV)[:, J:]
    sizes = [it[1] for it in items]
    got = _parser(match_on).parse_lowres(refined, tags, sizes)
    want = _one_by_one(_parser("host"), refined, tags, sizes)
    for n in range(4):
        _same(got[n], want[n])
        assert _n_people(got[n][0]) == items[n][2]
    assert np.array_equal(got[place][0], g["final"]) and len(g["final"]) == 2
    assert np.array_equal(np.array(got[place][1], np.float32), g["scores"])


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_equal_sizes_list_form_equals_tuple_form(nat, match_on):
    refined, tags = _mix_batch()
    r, t = refined.to(DEV), tags.to(DEV)
    for hw in ((256, 320), (128, 160), (100, 333)):
        for adjust, refine in ((True, True), (False, False)):
            want = _parser(match_on).parse_lowres(r, t, hw, adjust, refine)
            got = _parser(match_on).parse_lowres(r, t, [hw] * 8, adjust, refine)
            for n in range(8):
                _same(got[n], want[n])
                if hw == (256, 320):                                       # (the size the blobs were drawn for)
                    assert _n_people(want[n][0]) == MIX_P[n]
            assert sum(_n_people(w[0]) for w in want) >= 20


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_equal_sizes_at_the_bench_shape(nat, teacher, match_on):
    """32 x 640 x 640, W0 teacher outputs: noise maps on which every image reaches the 30-people cap"""
    from rtpe.engine import TeacherPipeline
    x = synth.make_images(32, 640, 640).to(DEV)
    pipe = TeacherPipeline(teacher, _parser(match_on), device=DEV)
    want = pipe(x, (640, 640))
    got = pipe(x, [(640, 640)] * 32)
    for n in range(32):
        _same(got[n], want[n])
        assert _n_people(want[n][0]) >= 30


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_empty_images_at_the_start_in_the_middle_and_at_the_end(nat, match_on):
    """pins the offsets of the compaction: people of image n follow those of the images before it"""
    refined, tags = _mix_batch()
    order = [1, 0, 2, 1, 1, 7, 3, 6, 1]                                    # image 1 has nobody
    refined, tags = refined[order].contiguous(), tags[order].contiguous()
    sizes = [MIX_HW[i] for i in order]
    for n, hw in ((0, (31, 47)), (3, (427, 640)), (4, (64, 80))):          # the empty ones at sizes of every kind
        sizes[n] = hw
    expect = [MIX_P[i] for i in order]
    assert expect == [0, 3, 5, 0, 0, 6, 2, 3, 0]
    got = _parser(match_on).parse_lowres(refined.to(DEV), tags.to(DEV), sizes)
    for n in range(9):
        want = _oracle(refined, tags, n, sizes[n])
        assert _n_people(want[0]) == expect[n], n
        _same(got[n], want)
    nobody = _parser(match_on).parse_lowres(torch.zeros_like(refined).to(DEV), tags.to(DEV), sizes)
    assert all(p.shape == (0,) and s == [] for p, s in nobody)


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_stream_with_a_size_callable_equals_call(nat, teacher, match_on):
    from rtpe.engine import TeacherPipeline
    pipe = TeacherPipeline(teacher, _parser(match_on), device=DEV)
    batches = [synth.make_images(3, 128, 160, seed=70 + k).to(DEV) for k in range(3)]
    sizes = [[(128, 160), (100, 150), (96, 120)], [(64, 80), (128, 160), (200, 250)], [(31, 47), (120, 90), (128, 131)]]
    call = [pipe(b, s) for b, s in zip(batches, sizes)]
    got = list(pipe.stream(iter(batches), lambda k: sizes[k]))
    mixed = list(pipe.stream(iter(batches), lambda k: sizes[k] if k != 1 else (64, 80)))
    assert len(got) == len(call) == 3
    one = TeacherPipeline(teacher, _parser("host"), device=DEV)
    for k in range(3):
        for n in range(3):
            _same(got[k][n], call[k][n])
            alone = one(batches[k][n:n + 1], sizes[k][n])[0]                # the one-size entry, the image alone
            _same(got[k][n], alone)
            assert _n_people(alone[0]) >= 1
            _same(mixed[k][n], alone if k != 1 else one(batches[k][n:n + 1], (64, 80))[0])
    # the refusals of stream(): a wrong count, and per-image sizes with the flip test
    with pytest.raises(ValueError):
        list(pipe.stream(iter(batches), lambda k: sizes[k][:2]))
    with pytest.raises(ValueError, match="per-image decode sizes"):
        list(TeacherPipeline(teacher, _parser(), device=DEV, flip_test=True).stream(iter(batches), lambda k: sizes[k]))


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("one_per_forward", [False, True])
def test_plain_inference_equals_the_per_image_loop(nat, teacher, match_on, one_per_forward):
    from rtpe import inference
    from rtpe.third_party import transforms
    shapes = [(192, 256), (180, 256), (256, 192), (150, 200), (192, 256), (256, 180)]
    rng = np.random.default_rng(7)
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    inputs = [transforms.get_multi_scale_size(img, 256, 1.0, 1)[0] for img in images]
    budget = max(w * h for w, h in inputs) if one_per_forward else None
    plan = inference.plain_plan(shapes, 256, 2, budget)
    assert [len(c) for c in plan] == ([1] * 6 if one_per_forward else [2, 2, 2])
    assert plan != inference.plain_plan(shapes, 256, 2, budget, by_original_size=True) or one_per_forward
    parser = _parser("host")
    got = inference.plain_inference(teacher, _parser(match_on), images, 256, 2, budget, device=DEV, match_on=match_on)
    assert len(got) == 6
    for img, res in zip(images, got):
        t, _, _ = transforms.warp_normalize(img, 256, 1, 1, device=DEV)
        with torch.no_grad():
            preds, refined = teacher(t)
        want = parser.parse_lowres(refined, preds[:, J:], img.shape[:2])[0]
        _same(res, want)
        assert _n_people(want[0]) >= 1
