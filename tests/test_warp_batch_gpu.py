"""Batched pre-processing on the GPU (``transforms.warp_normalize_batch``, the drivers' ``warp="batch"``): a whole chunk
of images at every test scale with one upload and one launch per scale.  The yardstick is never the new path: it is the
per-image entry ``transforms.warp_normalize`` (``torch.equal``, no image or scale left out), the numpy oracle of the
same arithmetic, and the drivers with ``warp="image"``."""
import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

J = 17
DEV = "cuda:0"
LANDSCAPE = [(96, 128), (90, 128), (100, 128), (97, 131)]       # input 128: all 192 x 128
PORTRAIT = [(128, 96), (131, 97), (128, 90)]                    # 128 x 192


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


def _images(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]


def _check_against_per_image(images, input_size, scales, sizes_wh, **kw):
    """every (image, scale) of one batched call against the per-image entry: bits, centre and scale"""
    from rtpe.third_party import transforms
    ts, centers, scale_arrays = transforms.warp_normalize_batch(images, input_size, scales, device=DEV, **kw)
    assert len(ts) == len(scales) and len(centers) == len(scale_arrays) == len(images)
    for s, (cs, ms) in enumerate(scales):
        w, h = sizes_wh[s]
        assert tuple(ts[s].shape) == (len(images), 3, h, w) and ts[s].dtype == torch.float32 and ts[s].is_contiguous()
        assert ts[s].device == torch.device(DEV)
        for n, img in enumerate(images):
            want, center, scale = transforms.warp_normalize(img, input_size, cs, ms, device=DEV, **kw)
            assert torch.equal(ts[s][n:n + 1], want), (s, n)
            assert np.array_equal(centers[n][s], center) and np.array_equal(scale_arrays[n][s], scale)
            assert centers[n][s].dtype == center.dtype and scale_arrays[n][s].dtype == scale.dtype
    return ts


@pytest.mark.parametrize("shapes, size", [(LANDSCAPE, (192, 128)), (PORTRAIT, (128, 192)), (LANDSCAPE[3:], (192, 128))])
@pytest.mark.parametrize("kw", [{}, {"round_u8": False},
                                {"mean": (0.1, 0.5, 0.9), "std": (0.3, 1.7, 0.05), "round_u8": True},
                                {"mean": (0.0, 0.0, 0.0), "std": (1 / 255., 1 / 255., 1 / 255.), "round_u8": False}])
def test_batch_warp_is_bit_identical_to_the_per_image_entry(nat, shapes, size, kw):
    ts = _check_against_per_image(_images(shapes, 11), 128, [(1, 1)], [size], **kw)
    assert float(ts[0].std()) > 0.1                                      # (a real image came out, not a constant)


def test_all_scales_in_one_call(nat):
    from rtpe.third_party import transforms
    images = _images(LANDSCAPE, 12)
    scales = [(2, .5), (1, .5), (.5, .5)]
    sizes = [(512, 256), (256, 128), (128, 64)]
    for img in images:                                                  # (checked here on the CPU)
        assert [transforms.get_multi_scale_size(img, 128, cs, ms)[0] for cs, ms in scales] == sizes
    _check_against_per_image(images, 128, scales, sizes)


def test_odd_widths(nat):
    """134 x 89: a width that is no multiple of 4 (rows of the planes start at every alignment), partial tiles in both
    directions, the last rows; every image of the landscape group, 97 x 131 among them"""
    ts = _check_against_per_image(_images(LANDSCAPE, 13), 128, [(0.7, 1)], [(134, 89)])
    assert bool(torch.isfinite(ts[0]).all())
    # and two scales of odd sizes in one call: 134 x 89 and 249 x 166
    _check_against_per_image(_images(LANDSCAPE, 14), 128, [(0.7, 1), (1.3, 1)], [(134, 89), (249, 166)])


def test_inputs_mixed(nat):
    """the same image as ndarray, CPU tensor and device tensor, and a device tensor with padded rows: the same bits"""
    from rtpe.third_party import transforms
    img = _images(LANDSCAPE[3:], 15)[0]
    want = transforms.warp_normalize(img, 128, device=DEV)[0]
    padded = torch.zeros((97, 400), dtype=torch.uint8, device=DEV)
    padded[:, :393] = torch.from_numpy(img).to(DEV).reshape(97, 393)
    rows = padded.as_strided((97, 131, 3), (400, 3, 1))
    forms = [img, torch.from_numpy(img.copy()), torch.from_numpy(img).to(DEV), rows, np.asfortranarray(img)]
    ts, _, _ = transforms.warp_normalize_batch(forms, 128, device=DEV)
    for n in range(len(forms)):
        assert torch.equal(ts[0][n:n + 1], want), n
    only_device, _, _ = transforms.warp_normalize_batch([forms[2], rows], 128, device=DEV)
    assert torch.equal(only_device[0][:1], want) and torch.equal(only_device[0][1:], want)


def test_ring_reuse(nat):
    """more consecutive calls than the ring has slots, each with other pixels, read only at the end"""
    from rtpe.third_party import transforms
    calls = 3 * transforms.WARP_RING_SLOTS + 1
    sets = [_images(LANDSCAPE, 100 + k) for k in range(calls)]
    got = [transforms.warp_normalize_batch(imgs, 128, [(1, 1), (0.7, 1)], device=DEV)[0] for imgs in sets]
    assert len(transforms._WARP_RING[0]["slots"]) == transforms.WARP_RING_SLOTS
    torch.cuda.synchronize()
    for imgs, ts in zip(sets, got):
        for s, (cs, ms) in enumerate([(1, 1), (0.7, 1)]):
            for n, img in enumerate(imgs):
                assert torch.equal(ts[s][n:n + 1], transforms.warp_normalize(img, 128, cs, ms, device=DEV)[0])


def test_batch_warp_vs_oracle(nat):
    """one batch against the numpy restatement of the same convention, within the bound of
    test_gpu_parity.test_warp_normalize_vs_oracle: the two 2x3 matrices (3-point solve vs closed form) agree to 1e-9 but
    may round differently to fp32, which moves a sampling position by one ulp; one grey level would be 1.7e-2"""
    from oracle import preprocess_ref
    from rtpe.third_party import transforms
    images = _images(LANDSCAPE, 16)
    ts, centers, _ = transforms.warp_normalize_batch(images, 128, device=DEV)
    for n, img in enumerate(images):
        want, center, _ = preprocess_ref.warp_normalize(img, 128, transforms.IMAGENET_MEAN, transforms.IMAGENET_STD)
        np.testing.assert_array_equal(center, centers[n][0])
        err = np.abs(ts[0][n].cpu().numpy() - want).max()
        assert err <= 2e-4, (n, err)


def _parser(match_on="host"):
    from rtpe.third_party.group import HeatmapParser
    return HeatmapParser(J, 30, 0.1, 1.0, True, False, True, 5, 2, match_on=match_on)


def _n_people(people):
    return len(people) if getattr(people, "ndim", 0) == 3 else 0


SHAPES = [(192, 256), (180, 256), (256, 192), (150, 200), (192, 256), (256, 180)]


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("one_per_forward", [False, True])
def test_plain_inference_warp_batch_equals_warp_image(nat, teacher, match_on, one_per_forward):
    from rtpe import inference
    from rtpe.third_party import transforms
    images = _images(SHAPES, 7)
    inputs = [transforms.get_multi_scale_size(img, 256, 1.0, 1)[0] for img in images]
    budget = max(w * h for w, h in inputs) if one_per_forward else None
    assert [len(c) for c in inference.plain_plan(SHAPES, 256, 2, budget)] == ([1] * 6 if one_per_forward else [2, 2, 2])
    want = inference.plain_inference(teacher, _parser(match_on), images, 256, 2, budget, device=DEV, match_on=match_on,
                                     warp="image")
    got = inference.plain_inference(teacher, _parser(match_on), images, 256, 2, budget, device=DEV, match_on=match_on,
                                    warp="batch")
    assert len(got) == len(want) == 6
    for (gp, gs), (wp, ws) in zip(got, want):
        assert _n_people(gp) == _n_people(wp)
        assert np.array_equal(np.asarray(gp, np.float32), np.asarray(wp, np.float32))
        assert np.array_equal(np.array(gs, np.float32), np.array(ws, np.float32))
    assert sum(_n_people(p) for p, _ in want) >= 1


@pytest.mark.parametrize("driver", ["flip", "multi_scale"])
def test_flip_and_multi_scale_warp_batch_equal_warp_image(nat, teacher, driver):
    from rtpe import inference
    images = _images(SHAPES, 7)
    if driver == "multi_scale":
        sizes = inference.multi_scale_input_sizes(images[0], 256, (2, 1, 0.5))
        assert sizes == ((768, 512), (384, 256), (192, 128))
        assert inference.multi_scale_input_sizes(images[2], 256, (2, 1, 0.5)) == ((512, 768), (256, 384), (128, 192))

    def run(warp):
        if driver == "flip":
            return inference.flip_test_inference(teacher, _parser(), images, input_size=256, batch_size=2, device=DEV,
                                                 warp=warp)
        return inference.multi_scale_batch_inference(teacher, _parser(), images, input_size=256, scale_factors=(2, 1, 0.5),
                                                     flip_test=True, batch_size=2, device=DEV, warp=warp)
    want, got = run("image"), run("batch")
    assert len(got) == len(want) == 6
    for (res, sc), (wres, wsc) in zip(got, want):
        assert len(res) == len(wres)
        for a, b in zip(res, wres):
            assert np.array_equal(a, b)
        assert np.array_equal(np.array(sc, np.float32), np.array(wsc, np.float32))
    assert sum(len(res) for res, _ in want) >= 1
