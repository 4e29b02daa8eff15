"""GPU tests of the one-pass decode of a mixed-size batch from its canvas (include/rtpe_hip_mixdec.h,
HeatmapParser.parse_lowres_mixed, StudentPipeline.call_mixed / stream_mixed).  Every comparison is exact: per image the
bits of the shared-tag decode of a contiguous copy of the image's region at the image's own size.  The batch, its seeds
and the two canvases are those of tests/test_mixed_decode_host.py; everything outside the regions is NaN."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_mixed_decode_host as MD
import test_student_sizes_host as S
from oracle import decode_ref, synth

pytestmark = pytest.mark.gpu

J = MD.J
DEV = "cuda:0"
SIZES, EXTENTS, CANVASES = MD.SIZES, MD.EXTENTS, MD.CANVASES
ALL_SIZES, ALL_EXTENTS = MD.ALL_SIZES, MD.ALL_EXTENTS        # + the two extra small images (6 and 7) of the tap-order test
COMBOS = [(True, True), (True, False), (False, True), (False, False)]
WINDOWS = [(5, 2, 30), (3, 1, 20), (7, 3, 12)]            # (NMS window, padding, K)
SMALL = [n for n, (h, w) in enumerate(SIZES) if h + w <= 128]


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


def _parser(match_on="host", K=30, ksize=5, pad=2):
    from rtpe.third_party.group import HeatmapParser
    return HeatmapParser(J, K, 0.1, 1.0, True, False, True, ksize, pad, match_on=match_on)


def _n_people(people):
    return len(people) if getattr(people, "ndim", 0) == 3 else 0


def _same(got, want):
    gp, gs = got
    wp, ws = want
    assert _n_people(gp) == _n_people(wp)
    assert np.array_equal(np.asarray(gp, np.float32), np.asarray(wp, np.float32))
    assert np.array_equal(np.array(gs, np.float32), np.array(ws, np.float32))


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# --------------------------------------------------------------------------- #
# ABI level: the three top-k tables
# --------------------------------------------------------------------------- #
_ALONE = {}


def _alone_tables(nat, n, window, tag_scale=1):
    """rtpe_topk_fused_shared on the contiguous region of image n at its own size (computed once per case) with the indices
    re-encoded from y * ow_n + x to y * w_enc + x"""
    key = (n, window, tag_scale)
    if key not in _ALONE:
        ksize, pad, K = window
        heat, tag = MD.region(n)[0].to(DEV), MD.region(n, tag_scale)[1].to(DEV)
        oh, ow = ALL_SIZES[n]
        L = nat.lib()
        nb = ctypes.c_size_t()
        nat.check(L.rtpe_topk_scratch_bytes(J, oh, ow, K, ctypes.byref(nb)))
        scratch = torch.empty(max(nb.value, 8), dtype=torch.uint8, device=DEV)
        val = torch.empty((1, J, K), dtype=torch.float32, device=DEV)
        ind = torch.empty((1, J, K), dtype=torch.int32, device=DEV)
        tg = torch.empty((1, J, K, 1), dtype=torch.float32, device=DEV)
        with torch.cuda.device(heat.device):
            nat.check(L.rtpe_topk_fused_shared(_p(heat), heat.shape[2], heat.shape[3], heat.stride(0), _p(tag), tag.shape[2],
                                               tag.shape[3], tag.stride(0), 1, J, oh, ow, K, ksize, pad, _p(val), _p(ind),
                                               _p(tg), _p(scratch), scratch.numel(), nat.stream_ptr(heat.device)))
        torch.cuda.synchronize()
        _ALONE[key] = (val.cpu().numpy()[0], ind.cpu().numpy()[0].astype(np.int64), tg.cpu().numpy()[0])
    return _ALONE[key]


def _mixed_tables(nat, heat, tag, order, window, tag_hw=None):
    """rtpe_decode_mixed_fill + rtpe_topk_fused_mixed on canvases (device tensors, possibly channel slices) -> numpy tables
    and w_enc"""
    ksize, pad, K = window
    L = nat.lib()
    N = len(order)
    assert heat.shape[:2] == (N, J) and tag.shape[:2] == (N, 1)
    assert heat.stride(1) == heat.shape[2] * heat.shape[3] and heat.stride(3) == 1 and tag.stride(3) == 1
    pairs = lambda hw: (ctypes.c_int32 * (2 * N))(*[v for p in hw for v in p])
    tab = torch.empty((16 * N,), dtype=torch.int32, pin_memory=True)
    mh, mw = ctypes.c_int32(), ctypes.c_int32()
    nat.check(L.rtpe_decode_mixed_fill(pairs([ALL_SIZES[n] for n in order]), pairs([ALL_EXTENTS[n] for n in order]),
                                       None if tag_hw is None else pairs(tag_hw), N, heat.shape[2], heat.shape[3],
                                       tag.shape[2], tag.shape[3], _p(tab), 64 * N, ctypes.byref(mh), ctypes.byref(mw)))
    assert (mh.value, mw.value) == (max(ALL_SIZES[n][0] for n in order), max(ALL_SIZES[n][1] for n in order))
    w_enc = mw.value
    tab_d = tab.to(DEV)
    nb = ctypes.c_size_t()
    nat.check(L.rtpe_topk_scratch_bytes(N * J, mh.value, mw.value, K, ctypes.byref(nb)))
    scratch = torch.empty(max(nb.value, 8), dtype=torch.uint8, device=DEV)
    val = torch.empty((N, J, K), dtype=torch.float32, device=DEV)
    ind = torch.empty((N, J, K), dtype=torch.int32, device=DEV)
    tg = torch.empty((N, J, K, 1), dtype=torch.float32, device=DEV)
    with torch.cuda.device(heat.device):
        nat.check(L.rtpe_topk_fused_mixed(_p(heat), heat.shape[2], heat.shape[3], heat.stride(0), _p(tag), tag.shape[2],
                                          tag.shape[3], tag.stride(0), N, J, _p(tab_d), 64 * N, mh.value, mw.value, w_enc,
                                          K, ksize, pad, _p(val), _p(ind), _p(tg), _p(scratch), scratch.numel(),
                                          nat.stream_ptr(heat.device)))
    torch.cuda.synchronize()
    return val.cpu().numpy(), ind.cpu().numpy().astype(np.int64), tg.cpu().numpy(), w_enc


def _tables_equal(nat, got, order, window, tag_scale=1):
    val, ind, tg, w_enc = got
    for i, n in enumerate(order):
        wv, wi, wt = _alone_tables(nat, n, window, tag_scale)
        ow = ALL_SIZES[n][1]
        assert np.array_equal(val[i], wv), (n, window)
        assert np.array_equal(ind[i], (wi // ow) * w_enc + wi % ow), (n, window)
        assert val[i].tobytes() == wv.tobytes() and tg[i].tobytes() == wt.tobytes(), (n, window)
        assert (wv > 0.1).sum() >= 3                              # candidates were found: no empty decode
        assert not np.isnan(tg[i]).any() and not np.isnan(val[i]).any()


@pytest.mark.parametrize("window", WINDOWS, ids=["5x5_K30", "3x3_K20", "7x7_K12"])
@pytest.mark.parametrize("canvas_hw", CANVASES, ids=["tight", "loose"])
def test_mixed_topk_tables_equal_those_of_every_region_alone(nat, canvas_hw, window):
    """both canvases, three windows; the heat and tag canvases are the channel slices of ONE det canvas"""
    det = MD.canvas_det(canvas_hw).to(DEV)
    assert bool(torch.isnan(det).any())
    order = list(range(len(SIZES)))
    _tables_equal(nat, _mixed_tables(nat, det[:, :J], det[:, J:], order, window), order, window)


def _tap_orders(nat, order, canvas_hw, small):
    """the mixed top-k of the batch ``order`` against F.interpolate on the CPU, on every tag plane expanded to J channels.  For
    every image of ``small`` (positions in the batch): EVERY joint-16 table entry carries channel 16's bits (the tail order of
    the small-output kernel), the candidates of joints 0 and 15 carry their own channel's (the other order).  Returns per
    position the number of joint-16 candidates whose bits differ between channel 16 and channel 0"""
    window = WINDOWS[0]
    d = MD.canvas_det(canvas_hw, order).to(DEV)
    val, ind, tg, w_enc = got = _mixed_tables(nat, d[:, :J], d[:, J:], order, window)
    _tables_equal(nat, got, order, window)
    differ = {}
    for i in small:
        oh, ow = ALL_SIZES[order[i]]
        assert oh + ow <= 128
        up = F.interpolate(MD.region(order[i])[1].expand(-1, J, -1, -1).contiguous(), (oh, ow), mode="bilinear",
                           align_corners=True)
        differ[i] = 0
        assert (val[i, 16] > 0.1).sum() >= 2
        for k in range(window[2]):
            y, x = divmod(int(ind[i, 16, k]), w_enc)
            assert y < oh and x < ow
            c16, c0 = up[0, 16, y, x].numpy(), up[0, 0, y, x].numpy()
            assert tg[i, 16, k, 0].tobytes() == c16.tobytes(), (i, k)          # the kernel took channel 16's order
            differ[i] += bool(val[i, 16, k] > 0.1) and c16.tobytes() != c0.tobytes()
        for j in (0, 15):                                                       # ... and the other order for the others
            for k in np.nonzero(val[i, j] > 0.1)[0]:
                y, x = divmod(int(ind[i, j, k]), w_enc)
                assert tg[i, j, k, 0].tobytes() == up[0, j, y, x].numpy().tobytes(), (i, j, k)
    print("joint-16 candidates whose tag bits differ between channel 16 and channel 0:", differ)
    return differ


def test_mixed_topk_takes_the_tap_order_of_channel_16_for_the_small_images(nat):
    """The small images of the batch (oh + ow <= 128) are sampled with the small-output kernel's arithmetic, joint 16 in
    the tail order (``_tap_orders``).

    Which candidates differ between the two orders is a property of the inputs alone (CPU): in 33 x 47 and 47 x 33 one axis
    has the scale 8 / 32 = 1 / 4 exactly, the local maxima of the upsampled maps sit on rows / columns that coincide with a
    source row / column, there one axis weight pair is (1, 0) and both tap orders give the same bits - none of their
    joint-16 table entries differs, under any of the three windows (0 of 30 / 20 / 12 entries each).  64 x 64 has 2 differing
    candidates.  So for this batch the difference itself is asserted for 64 x 64; a landscape and a portrait image whose
    candidates do differ are in the next test."""
    differ = _tap_orders(nat, list(range(len(SIZES))), CANVASES[1], SMALL)
    assert differ == {3: 0, 4: 0, 5: 2}


@pytest.mark.parametrize("canvas_hw", CANVASES, ids=["tight", "loose"])
def test_mixed_topk_tap_order_of_a_landscape_and_a_portrait_small_image(nat, canvas_hw):
    """38 x 58 and 58 x 38 (seed 58) between two images of the batch, one of them large: in each of the two a joint-16
    candidate's tag bits differ between channel 16 and channel 0 (1 and 2 of 3 candidates, known from the CPU), and the
    kernel returned channel 16's - in both orientations, beside images that take the other sample kernel"""
    differ = _tap_orders(nat, [0, 6, 4, 7], canvas_hw, [1, 2, 3])
    assert differ[1] >= 1 and differ[3] >= 1
    assert differ == {1: 1, 2: 0, 3: 2}


def test_mixed_topk_with_the_tag_canvas_at_half_the_heat_maps_resolution(nat):
    """the tag canvas has its own pitch and every image its own tag extents (ceil(extent / 2)): the table's tag axes"""
    order = list(range(len(SIZES)))
    heat = MD.canvas_det(CANVASES[1])[:, :J].contiguous().to(DEV)
    tag_hw = [(-(-eh // 2), -(-ew // 2)) for eh, ew in EXTENTS]
    tag = torch.full((len(order), 1, 15, 20), float("nan"))
    for n in order:
        tag[n, 0, :tag_hw[n][0], :tag_hw[n][1]] = MD.region(n, 2)[1][0, 0]
    for window in WINDOWS[:2]:
        _tables_equal(nat, _mixed_tables(nat, heat, tag.to(DEV), order, window, tag_hw), order, window, 2)


@pytest.mark.parametrize("n", [0, 3])
def test_mixed_topk_of_one_image(nat, n):
    det = MD.canvas_det(CANVASES[1], [n]).to(DEV)
    _tables_equal(nat, _mixed_tables(nat, det[:, :J], det[:, J:], [n], WINDOWS[0]), [n], WINDOWS[0])


# --------------------------------------------------------------------------- #
# the parser
# --------------------------------------------------------------------------- #
_PARSED = {}


def _parsed_alone(n, adjust, refine, match_on, blank=False):
    """parse_lowres_shared on a contiguous copy of image n's region at its own size (computed once per case)"""
    key = (n, adjust, refine, match_on, blank)
    if key not in _PARSED:
        heat, tag = MD.region(n)
        heat = torch.zeros_like(heat) if blank else heat
        res = _parser(match_on).parse_lowres_shared(heat.to(DEV), tag.to(DEV), SIZES[n], adjust, refine)
        assert len(res) == 1
        _PARSED[key] = res[0]
    return _PARSED[key]


def _not_empty(results, order):
    for i, n in enumerate(order):
        assert _n_people(results[i][0]) == MD.PEOPLE[n], (n, _n_people(results[i][0]))
        assert results[i][0].shape[1:] == (J, 4) and results[i][0].dtype == np.float32


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("canvas_hw", CANVASES, ids=["tight", "loose"])
def test_parse_lowres_mixed_equals_parse_lowres_shared_on_every_region(nat, canvas_hw, match_on):
    det = MD.canvas_det(canvas_hw).to(DEV)
    order = list(range(len(SIZES)))
    for adjust, refine in COMBOS:
        got = _parser(match_on).parse_lowres_mixed(det, SIZES, adjust, refine)
        assert len(got) == len(SIZES)
        for n in order:
            _same(got[n], _parsed_alone(n, adjust, refine, match_on))
        _not_empty(got, order)
    # the pair form: slices of the canvas, and a three-dimensional tag; the state is that of the per-image sizes
    p = _parser(match_on)
    st = p.lowres_topk_mixed((det[:, :J], det[:, J]), SIZES)
    assert st["refine"][0] == "rtpe_adjust_refine_fused_mixed_topk" and st["refine"][2] is True and st["D"] == 1
    assert st["w_enc"] == 140 and st["hw"] == (100, 140) and st["sizes"][1] == SIZES
    assert st["refined"].data_ptr() == det.data_ptr() and st["tags"].data_ptr() == det[:, J:].data_ptr()     # no copies
    p.lowres_match(st)
    got = p.lowres_finish(st)
    for n in order:
        _same(got[n], _parsed_alone(n, True, True, match_on))


def test_parse_lowres_mixed_equals_the_cpu_oracle(nat):
    """upsample every image's own maps (the tag plane expanded) with the stock CPU op, then the oracle's parse"""
    got = _parser().parse_lowres_mixed(MD.canvas_det(CANVASES[1]).to(DEV), SIZES)
    for n, (oh, ow) in enumerate(SIZES):
        heat, tag = MD.region(n)
        hms = decode_ref.upsample_bilinear(heat, oh, ow)
        aes = decode_ref.upsample_bilinear(tag.expand(-1, J, -1, -1).contiguous(), oh, ow)
        want, wsc = decode_ref.HeatmapParserRef().parse(hms, aes.unsqueeze(-1))
        assert _n_people(want[0]) == MD.PEOPLE[n]
        _same(got[n], (want[0], wsc))


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_parse_lowres_mixed_does_not_depend_on_the_order_of_the_batch(nat, match_on):
    order = list(range(len(SIZES)))[::-1]
    got = _parser(match_on).parse_lowres_mixed(MD.canvas_det(CANVASES[1], order).to(DEV), [SIZES[n] for n in order])
    for i, n in enumerate(order):
        _same(got[i], _parsed_alone(n, True, True, match_on))
    _not_empty(got, order)


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_parse_lowres_mixed_with_all_zero_heat_maps_at_the_start_in_the_middle_and_at_the_end(nat, match_on):
    order = list(range(len(SIZES)))
    blank = (0, 2, 5)
    got = _parser(match_on).parse_lowres_mixed(MD.canvas_det(CANVASES[1], order, blank).to(DEV), SIZES)
    for n in order:
        if n in blank:
            assert _n_people(got[n][0]) == 0 and len(got[n][1]) == 0
            _same(got[n], _parsed_alone(n, True, True, match_on, blank=True))
        else:
            _same(got[n], _parsed_alone(n, True, True, match_on))
            assert _n_people(got[n][0]) == MD.PEOPLE[n]


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_parse_lowres_mixed_of_equal_sizes_equals_parse_lowres_shared_on_the_batch(nat, match_on):
    """extent == pitch for every image: the table is that of the per-image sizes, the batch that of parse_lowres_shared"""
    for hw, src in (((64, 96), (16, 24)), ((64, 64), (16, 16))):            # (the second: a small output)
        sets = [synth.make_decode_maps(3, src[0], src[1], seed=s, sigma=1.0) for s in (52, 53, 51)]
        heat = torch.from_numpy(np.concatenate([s[0] for s in sets]))
        tag = torch.from_numpy(np.concatenate([s[1][..., 0] for s in sets])).amax(1, keepdim=True)
        det = torch.cat([heat, tag], 1).contiguous().to(DEV)
        want = _parser(match_on).parse_lowres_shared(det[:, :J], det[:, J:], hw)
        got = _parser(match_on).parse_lowres_mixed(det, [hw] * 3)
        assert len(got) == 3
        for g, w in zip(got, want):
            _same(g, w)
        assert sum(_n_people(g[0]) for g in got) >= 9


# (maps, decode size): the small-output sampler (oh + ow <= 128) with one boundary of the 32 x 64 top-k tile in each direction;
# the other sampler with more than one tile both ways
FOUR_PATHS = [((10, 18), (40, 72)), ((18, 34), (72, 136))]


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("src,hw", FOUR_PATHS, ids=["40x72_small_output", "72x136"])
def test_the_four_public_paths_agree_on_equal_sizes_with_one_tag_plane(nat, src, hw, match_on):
    """the two switches of the network-output kind (one tag plane per image; sizes from the table), all four
    combinations on the same maps: every image has the same size and every extent is the pitch, so each path must return
    the rows and scores of the plain decode of the tag plane expanded to J channels"""
    sets = [synth.make_decode_maps(3, src[0], src[1], seed=s, sigma=1.0) for s in (61, 62, 63)]
    heat = torch.from_numpy(np.concatenate([s[0] for s in sets]))
    tag = torch.from_numpy(np.concatenate([s[1][..., 0] for s in sets])).amax(1, keepdim=True)
    det = torch.cat([heat, tag], 1).contiguous().to(DEV)
    heat, tag = det[:, :J].contiguous(), det[:, J:]
    expanded = tag.expand(-1, J, -1, -1).contiguous()
    want = _parser(match_on).parse_lowres(heat, expanded, hw)
    assert len(want) == 3 and all(_n_people(w[0]) >= 1 for w in want)
    paths = {"sizes": _parser(match_on).parse_lowres(heat, expanded, [hw] * 3),
             "shared": _parser(match_on).parse_lowres_shared(det[:, :J], tag, hw),
             "mixed": _parser(match_on).parse_lowres_mixed(det, [hw] * 3)}
    for name, got in paths.items():
        assert len(got) == 3, name
        for g, w in zip(got, want):
            _same(g, w)


def test_parse_lowres_mixed_records_equal_the_records_of_every_image(nat):
    from rtpe.engine import RECORD_FLOATS, unpack_records
    ids = [7, 1 << 24, 0, 12, 99, 5]
    det = MD.canvas_det(CANVASES[1]).to(DEV)
    rec = _parser("device").parse_lowres_mixed(det, SIZES, records=(ids, None))
    assert rec.is_cuda and rec.shape == (len(SIZES), RECORD_FLOATS) and rec.dtype == torch.float32
    for n in range(len(SIZES)):
        heat, tag = MD.region(n)
        want = _parser("device").parse_lowres_shared(heat.to(DEV), tag.to(DEV), SIZES[n], records=([ids[n]], None))
        assert torch.equal(rec[n:n + 1], want), n
    lists = _parser("device").parse_lowres_mixed(det, SIZES)
    back = unpack_records(rec)
    for n in range(len(SIZES)):
        assert len(back[ids[n]][0]) == MD.PEOPLE[n]
        assert np.array_equal(back[ids[n]][0], lists[n][0]) and np.array_equal(back[ids[n]][1], np.array(lists[n][1], np.float32))


# --------------------------------------------------------------------------- #
# the real seeded student: the tables from its det canvas
# --------------------------------------------------------------------------- #
def test_topk_tables_from_the_det_canvas_of_forward_mixed(nat, golden_dir):
    """forward_mixed on four of the sizes, then the top-k from its det canvas against the top-k of every region alone.  (A
    seeded network finds no people; the tables pad with zero-valued pixels in index order, so they are never empty.)"""
    from rtpe.students import AttentionStudent, pack_mixed, unpack_mixed
    order = [0, 1, 3, 4]
    stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False).eval()
    stu.load_state_dict(S.student_sd(golden_dir, "s100"), strict=True)
    stu = stu.to(DEV)
    ims = [synth.make_images(1, SIZES[n][0], SIZES[n][1], seed=80 + n)[0].to(DEV) for n in order]
    canvas, sizes = pack_mixed(ims)
    with torch.no_grad():
        att, det = stu.forward_mixed(canvas, sizes)
    assert det.shape == (4, J + 1, 25, 35) and det.dtype == torch.float32
    got = _mixed_tables(nat, det[:, :J], det[:, J:], order, WINDOWS[0])
    val, ind, tg, w_enc = got
    L = nat.lib()
    for i, (_, d) in enumerate(unpack_mixed(att, det, sizes)):
        d = d.unsqueeze(0).contiguous()
        n = order[i]
        oh, ow = SIZES[n]
        K = WINDOWS[0][2]
        nb = ctypes.c_size_t()
        nat.check(L.rtpe_topk_scratch_bytes(J, oh, ow, K, ctypes.byref(nb)))
        scratch = torch.empty(max(nb.value, 8), dtype=torch.uint8, device=DEV)
        wv = torch.empty((1, J, K), dtype=torch.float32, device=DEV)
        wi = torch.empty((1, J, K), dtype=torch.int32, device=DEV)
        wt = torch.empty((1, J, K, 1), dtype=torch.float32, device=DEV)
        heat, tag = d[:, :J], d[:, J:]
        with torch.cuda.device(d.device):
            nat.check(L.rtpe_topk_fused_shared(_p(heat), d.shape[2], d.shape[3], heat.stride(0), _p(tag), d.shape[2],
                                               d.shape[3], tag.stride(0), 1, J, oh, ow, K, 5, 2, _p(wv), _p(wi), _p(wt),
                                               _p(scratch), scratch.numel(), nat.stream_ptr(d.device)))
        torch.cuda.synchronize()
        wv, wi, wt = wv.cpu().numpy()[0], wi.cpu().numpy()[0].astype(np.int64), wt.cpu().numpy()[0]
        assert val[i].tobytes() == wv.tobytes() and tg[i].tobytes() == wt.tobytes(), n
        assert np.array_equal(ind[i], (wi // ow) * w_enc + wi % ow), n
        assert len(np.unique(ind[i][0])) == K                       # a full table of distinct pixels


# --------------------------------------------------------------------------- #
# StudentPipeline with a blob stand-in
# --------------------------------------------------------------------------- #
class _BlobMixed(torch.nn.Module):
    """``forward_mixed`` of a student that finds people: the det canvas of the batch at 1/4 of the input canvas, image n's
    maps (looked up by its size) in its region, NaN outside; fresh tensors on every call (the decode reads them on another
    stream)"""

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward_mixed(self, canvas, sizes):
        from rtpe import _native
        self.calls += 1
        order = [SIZES.index(tuple(hw)) for hw in sizes]
        hw = (_native.extent(canvas.shape[2], 2), _native.extent(canvas.shape[3], 2))
        det = MD.canvas_det(hw, order).to(canvas.device)
        return det[:, :1].sigmoid(), det


def _images(order):
    return [torch.zeros((3,) + SIZES[n], device=DEV) for n in order]


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_call_mixed_decodes_the_batch_in_one_pass_and_agrees_with_the_per_image_loop(nat, match_on):
    from rtpe.engine import RECORD_FLOATS, StudentPipeline
    order = [2, 5, 0, 3, 4, 1]
    pipe = StudentPipeline(_BlobMixed(), _parser(match_on), DEV)
    got = pipe.call_mixed(_images(order))
    loop = pipe.call_mixed(_images(order), decode="per_image")
    assert len(got) == len(loop) == 6 and pipe.model.calls == 2
    for i, n in enumerate(order):
        _same(got[i], loop[i])
        _same(got[i], _parsed_alone(n, True, True, match_on))
    _not_empty(got, order)
    if match_on == "device":
        ids = [3, 1, 4, 15, 9, 2]
        recs = pipe.call_mixed(_images(order), image_ids=ids)
        want = pipe.call_mixed(_images(order), image_ids=ids, decode="per_image")
        assert len(recs) == 6
        for r, w in zip(recs, want):
            assert r.shape == (1, RECORD_FLOATS) and torch.equal(r, w)
        assert recs[1].data_ptr() == recs[0].data_ptr() + 4 * RECORD_FLOATS      # views of the one record tensor


STREAM_ORDERS = [[0, 3, 5], [4, 1], [2, 5, 3, 0]]


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("in_flight", [1, 2])
def test_stream_mixed_equals_call_mixed_on_every_batch(nat, in_flight, match_on):
    from rtpe.engine import StudentPipeline
    from rtpe.students import pack_mixed
    pipe = StudentPipeline(_BlobMixed(), _parser(match_on), DEV)
    want = [pipe.call_mixed(_images(o)) for o in STREAM_ORDERS]
    # lists of images, and one (canvas, sizes) pair in a canvas larger than its images
    batches = [_images(STREAM_ORDERS[0]), pack_mixed(_images(STREAM_ORDERS[1]), (108, 152)), _images(STREAM_ORDERS[2])]
    got = list(pipe.stream_mixed(iter(batches), in_flight=in_flight))
    assert len(got) == 3
    for k, o in enumerate(STREAM_ORDERS):                           # in order
        assert len(got[k]) == len(o)
        for i, n in enumerate(o):
            _same(got[k][i], want[k][i])
            _same(got[k][i], _parsed_alone(n, True, True, match_on))
        _not_empty(got[k], o)
    if match_on == "device":
        recs = list(pipe.stream_mixed(iter(batches), in_flight=in_flight,
                                      records=lambda k: ([10 * k + i for i in range(len(STREAM_ORDERS[k]))], None)))
        for k, o in enumerate(STREAM_ORDERS):
            w = pipe.call_mixed(_images(o), image_ids=[10 * k + i for i in range(len(o))])
            assert torch.equal(recs[k], torch.cat(w))
    # stream() keeps refusing such batches
    with pytest.raises(ValueError, match="use call_mixed"):
        next(pipe.stream(iter(batches)))
    torch.cuda.synchronize()


def test_stream_mixed_stopped_early_leaves_the_stream_synchronised(nat):
    from rtpe.engine import StudentPipeline
    pipe = StudentPipeline(_BlobMixed(), _parser(), DEV)
    gen = pipe.stream_mixed(iter([_images(o) for o in STREAM_ORDERS]), in_flight=2)
    first = next(gen)
    gen.close()                                                     # three batches were submitted, one was taken
    for i, n in enumerate(STREAM_ORDERS[0]):
        _same(first[i], _parsed_alone(n, True, True, "host"))
    again = pipe.call_mixed(_images(STREAM_ORDERS[0]))              # on the main stream, right behind the closed loop
    for i, n in enumerate(STREAM_ORDERS[0]):
        _same(again[i], _parsed_alone(n, True, True, "host"))
    torch.cuda.synchronize()
