"""The order among equal values on every top-k and arg-max path of the HIP decode: ties go to the lowest flat index
(include/rtpe_hip.h ``rtpe_topk``, the header of csrc/decode.hip, include/rtpe_hip_sizes.h).  ``torch.topk`` leaves
that order undefined, so the yardstick is the oracle's stable top-k (``HeatmapParserRef(stable_topk=True)``, tied to the
reference in tests/test_decode_ties_host.py); ``np.argmax`` in its ``refine`` is first-occurrence already.

The inputs (oracle/ties.py) carry exact ties: equal maxima in one tile, across tiles and tile rows; a tie group at the
K-th place; plateaus of more than 512 local maxima in one tile and across a tile corner; planes of more than 2,048
tiles; a plane maximum at several pixels of different row stripes; equal refine scores from different heat values;
quarter-pixel steps without a larger neighbour in the interior, on every border and in the corners; negative values,
both zeros and the zero padding behind a tie group.  Every test first counts those structures on the CPU result
(``check_structure``), then compares EVERY element of what the GPU returns - zero-padding rows included - with the
oracle, bit for bit (+0 and -0 are the same value: the reference compares them equal and so does the contract)."""
import numpy as np
import pytest
import torch

from oracle import ties
from test_decode_ties_host import SIZES, TIE_CASES, case_ref, check_structure

pytestmark = pytest.mark.gpu

J = 17
SWITCHES = ((True, True), (False, True), (True, False), (False, False))      # (adjust, refine)
MATCH_ON = ("host", "device")


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


def _parser(c, match_on="host"):
    from rtpe.third_party.group import HeatmapParser
    par = HeatmapParser(J, c["K"], 0.1, 1.0, True, False, c.get("tag_per_joint", True), c.get("ksize", 5),
                        c.get("pad", 2), match_on=match_on)
    par.params.num_joints = c.get("J", J)
    return par


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=str(what))
    if got.dtype.kind == "f" and got.size:                   # bit for bit once -0 is folded onto +0
        a, b = (got.astype(np.float32) + np.float32(0)), (want.astype(np.float32) + np.float32(0))
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), what


def _same_people(got, want, what):
    """(people, scores) of one image against the oracle's (ans[0], scores)"""
    _same(got[0], want[0], (what, "people"))
    _same(np.array(got[1], np.float32), np.array(want[1], np.float32), (what, "scores"))


_ORACLE = {}


def _oracle(key, c, hms, aes, adjust, refine):
    """the stable oracle's ``parse`` of one image's upsampled maps -> (people, scores); computed once per key"""
    key = (key, adjust, refine)
    if key not in _ORACLE:
        ans, scores = case_ref(c).parse(hms, aes, adjust, refine)
        _ORACLE[key] = (ans[0], scores)
    return _ORACLE[key]


def _cuda(*ts):
    return [t.to("cuda:0") for t in ts]


# --------------------------------------------------------------------------- #
# already-upsampled maps: rtpe_topk (DirectMap), match, adjust, refine, parse
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("match_on", MATCH_ON)
@pytest.mark.parametrize("name", ["designed_k1", "designed_k30", "designed_k64", "designed_k30_d2", "designed_k30_3x3",
                                  "designed_k30_9x9"])
def test_top_k_and_parse_on_upsampled_maps(nat, name, match_on):
    c = TIE_CASES[name]()
    counts = check_structure(c)
    print(name, counts)
    # parse() below has no top-k table to hand to refine: every plane maximum comes from the plane-maximum pass on its
    # walk over flat indices, where one thread meets several of a plane's equal maxima in one stripe
    assert c["K"] < 30 or counts["efg"]["same_thread"]["flat"] >= 1
    ref, par = case_ref(c), _parser(c, match_on)
    det, tag = c["hms"], c["aes"]
    det_d, tag_d = _cuda(det, tag)
    want, got = ref.top_k(det, tag), par.top_k(det_d, tag_d)
    for k in ("val_k", "loc_k", "tag_k"):
        _same(got[k], want[k], (name, k))
    want_m, got_m = ref.match(**want), par.match(**got)
    assert len(got_m) == len(want_m) == 1
    _same(got_m[0], want_m[0], (name, "matched"))
    _same(par.adjust([m.copy() for m in got_m], det_d)[0], ref.adjust([m.copy() for m in want_m], det.numpy())[0],
          (name, "adjusted"))
    for a, r in SWITCHES:
        ans, scores = par.parse(det_d, tag_d, adjust=a, refine=r)
        assert len(ans) == 1
        _same_people((ans[0], scores), _oracle(name, c, det, tag, a, r), (name, a, r))
    # refine() for single people: the first three and the last of the adjusted rows
    adjusted = ref.adjust([m.copy() for m in want_m], det.numpy())[0]
    tag_np = tag[0].numpy()
    for p in sorted(set([0, 1, 2, len(adjusted) - 1]) & set(range(len(adjusted)))):
        one = par.refine(det[0], tag[0], adjusted[p].copy())
        _same(one, ref.refine(det[0].numpy(), tag_np, adjusted[p].copy()), (name, "refine", p))


@pytest.mark.parametrize("K", [8, 30])
def test_top_k_on_planes_of_more_than_2048_tiles(nat, K):
    """2,209 tiles per plane: the list scan of the merge, from its LDS copy (K = 8: 138 KiB of keys) and from
    global memory (K = 30: 518 KiB), with tie groups inside the top K, at the K-th place and before the padding"""
    c = TIE_CASES["big_k%d" % K]()
    print(K, check_structure(c))
    want = case_ref(c).top_k(c["hms"], c["aes"])
    got = _parser(c).top_k(*_cuda(c["hms"], c["aes"]))
    for k in ("val_k", "loc_k", "tag_k"):
        _same(got[k], want[k], (K, k))


# --------------------------------------------------------------------------- #
# the fused entry: rtpe_topk_fused (BilinearMap) + adjust / refine with the top-k table
# --------------------------------------------------------------------------- #
LOWRES = {"lowres_identity_k30": (30, False, 5, 2), "lowres_scaled_k30": (30, True, 5, 2),
          "lowres_scaled_k64": (64, True, 5, 2), "lowres_identity_k1": (1, False, 5, 2),
          "lowres_scaled_k30_3x3": (30, True, 3, 1), "lowres_identity_k30_9x9": (30, False, 9, 4)}


def _lowres_hw(scaled):
    return (319, 447) if scaled else ties.DIRECT_HW


@pytest.mark.parametrize("match_on", MATCH_ON)
@pytest.mark.parametrize("name", sorted(LOWRES))
def test_parse_lowres(nat, name, match_on):
    K, scaled, ksize, pad = LOWRES[name]
    c = TIE_CASES[name]()
    print(name, check_structure(c))
    refined, tags = ties.lowres_inputs(K)
    rd, td = _cuda(refined, tags)
    par = _parser(c, match_on)
    for a, r in SWITCHES:
        res = par.parse_lowres(rd, td, _lowres_hw(scaled), adjust=a, refine=r)
        assert len(res) == 1
        _same_people(res[0], _oracle(name, c, c["hms"], c["aes"], a, r), (name, a, r))


@pytest.mark.parametrize("name", ["lowres_identity_k30", "lowres_scaled_k30"])
def test_parse_lowres_with_the_plane_maximum_pass(nat, monkeypatch, name):
    """RTPE_REFINE_TOPK=0: refine's plane maxima come from ``plane_argmax_kernel`` (20 row stripes merged by
    atomicMax, staged source rows) instead of the top-k table; tied maxima must still resolve to the first pixel,
    also where one thread of that pass meets several of them in its columns of one stripe"""
    monkeypatch.setenv("RTPE_REFINE_TOPK", "0")
    K, scaled, _, _ = LOWRES[name]
    c = TIE_CASES[name]()
    assert check_structure(c)["efg"]["same_thread"]["column"] >= 1
    rd, td = _cuda(*ties.lowres_inputs(K))
    res = _parser(c).parse_lowres(rd, td, _lowres_hw(scaled))
    _same_people(res[0], _oracle(name, c, c["hms"], c["aes"], True, True), name)


@pytest.mark.parametrize("match_on", MATCH_ON)
def test_parse_lowres_with_one_size_per_image(nat, match_on):
    """rtpe_topk_fused_sizes: images smaller than the batch's largest (48 x 80 is at the small-output kernel's
    threshold, 48 + 80 <= 128); every image equals the one-size call on it alone and the oracle at its own size"""
    refined, tags = ties.sizes_inputs()
    rd, td = _cuda(refined, tags)
    cases = [TIE_CASES["sizes_%d" % n]() for n in range(4)]
    for n in range(4):
        print(n, SIZES[n], check_structure(cases[n]))
    assert SIZES[1][0] + SIZES[1][1] <= 128 and max(s[0] for s in SIZES) > SIZES[1][0]
    par = _parser(cases[0], match_on)
    for a, r in SWITCHES:
        res = par.parse_lowres(rd, td, SIZES, adjust=a, refine=r)
        assert len(res) == 4
        for n in range(4):
            alone = par.parse_lowres(rd[n:n + 1], td[n:n + 1], SIZES[n], adjust=a, refine=r)
            _same_people(res[n], alone[0], ("alone", n, a, r))
            _same_people(res[n], _oracle(("sizes", n), cases[n], cases[n]["hms"], cases[n]["aes"], a, r), (n, a, r))


# --------------------------------------------------------------------------- #
# flip and multi-scale tests: FlipHeatMap, MultiScaleHeatMap, the AGS tag plane
# --------------------------------------------------------------------------- #
def _net_case(scales, flip, ags):
    if scales == (1,) and flip and not ags:
        name = "flip"                                            # the single-scale flip test: parse_flip's inputs
    else:
        name = "ms%d%s%s" % (len(scales), "_flip" if flip else "", "_ags" if ags else "")
    return name, TIE_CASES[name]()


def _net_oracle(name, c, outs, scales, flip, ags, n, a, r):
    key = (name, n, a, r)
    if key not in _ORACLE:
        hms, aes = ties.net_maps(outs, scales, flip, n, ags)
        ans, scores = case_ref(c).parse(hms, aes, a, r)
        _ORACLE[key] = (ans[0], scores)
    return _ORACLE[key]


@pytest.mark.parametrize("match_on", MATCH_ON)
def test_parse_flip(nat, match_on):
    name, c = _net_case((1,), True, False)
    print(name, check_structure(c))
    outs = ties.net_outputs(2, (1,), seed=3)
    P, R, Pf, Rf = _cuda(*outs[0])
    par = _parser(c, match_on)
    for a, r in SWITCHES:
        res = par.parse_flip(P, R, Pf, Rf, ties.NET_HW, adjust=a, refine=r)
        assert len(res) == 2
        for n in range(2):
            _same_people(res[n], _net_oracle(name, c, outs, (1,), True, False, n, a, r), (name, n, a, r))
            assert res[n][0].shape[1:] == (J, 5)


@pytest.mark.parametrize("match_on", MATCH_ON)
@pytest.mark.parametrize("ags", [False, True], ids=["tags", "ags"])
@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
@pytest.mark.parametrize("scales", [(2, 1, 0.5), (1,)], ids=["s3", "s1"])
def test_parse_multi_scale(nat, scales, flip, ags, match_on):
    name, c = _net_case(scales, flip, ags)
    print(name, check_structure(c))
    outs = ties.net_outputs(2, scales, seed=3)
    dev = [_cuda(*(o if flip else o[:2])) for o in outs]
    par = _parser(dict(c, tag_per_joint=True), match_on)          # (the AGS branch does not read tag_per_joint)
    for a, r in SWITCHES:
        res = par.parse_multi_scale(dev, ties.NET_HW, scales, flip, adjust=a, refine=r, ags=ags)
        assert len(res) == 2
        for n in range(2):
            _same_people(res[n], _net_oracle(name, c, outs, scales, flip, ags, n, a, r), (name, n, a, r))
            assert res[n][0].shape[1:] == (J, 4 + int(flip and not ags))


# --------------------------------------------------------------------------- #
# the place in the batch, and the pipelined loop
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("match_on", MATCH_ON)
def test_the_place_in_the_batch_does_not_change_the_rows(nat, match_on):
    name = "lowres_identity_k30"
    c = TIE_CASES[name]()
    print(name, check_structure(c))
    seeds = (0, 1, 2, 3, 0, 5, 6, 7, 0)                            # the scene of the case first, in the middle, last
    rd, td = _cuda(*ties.lowres_inputs(30, seeds))
    par = _parser(c, match_on)
    for a, r in SWITCHES:
        want = _oracle(name, c, c["hms"], c["aes"], a, r)
        alone = par.parse_lowres(rd[:1], td[:1], ties.DIRECT_HW, adjust=a, refine=r)
        _same_people(alone[0], want, ("alone", a, r))
        res = par.parse_lowres(rd, td, ties.DIRECT_HW, adjust=a, refine=r)
        assert len(res) == 9
        for n in (0, 4, 8):
            _same_people(res[n], want, (n, a, r))
        assert all(len(p) > 0 for p, _ in res)


class _TieNet(torch.nn.Module):
    """a stand-in for the teacher: the input carries its batch number, the outputs are that batch's tie maps
    (fresh tensors on every call, as a forward pass returns them)"""

    def __init__(self, outs):
        super().__init__()
        self.outs = outs

    def forward(self, x):
        preds, refined = self.outs[int(x[0, 0, 0, 0].item())]
        return preds.clone(), refined.clone()


@pytest.mark.parametrize("match_on", MATCH_ON)
def test_pipeline_call_equals_stream_on_tie_maps(nat, match_on):
    """TeacherPipeline.__call__ and .stream() with the network outputs replaced by tie maps (the engine is not
    touched: the pipeline takes any module as its model)"""
    from rtpe.engine import TeacherPipeline
    name = "lowres_identity_k30"
    c = TIE_CASES[name]()
    check_structure(c)
    seeds = ((0, 1, 2), (3, 0, 4), (5, 6, 0))
    outs = []
    for sd in seeds:
        refined, tags = ties.lowres_inputs(30, sd)
        preds = torch.zeros((len(sd), 2 * J) + tuple(tags.shape[2:]))
        preds[:, J:] = tags
        outs.append(tuple(_cuda(preds, refined)))
    H, W = 2 * ties.DIRECT_HW[0], 2 * ties.DIRECT_HW[1]
    batches = [torch.full((3, 3, H, W), float(k), device="cuda:0") for k in range(3)]
    pipe = TeacherPipeline(_TieNet(outs), _parser(c), device="cuda:0", match_on=match_on)
    want = [pipe(b, out_hw=ties.DIRECT_HW) for b in batches]
    got = list(pipe.stream(iter(batches), out_hw=ties.DIRECT_HW))
    assert len(got) == len(want) == 3
    oracle = _oracle(name, c, c["hms"], c["aes"], True, True)
    for k in range(3):
        assert len(got[k]) == len(want[k]) == 3
        for n in range(3):
            _same_people(got[k][n], want[k][n], ("stream", k, n))
            if seeds[k][n] == 0:
                _same_people(want[k][n], oracle, ("call", k, n))
