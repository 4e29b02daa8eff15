"""The shared-tag plain decode and ``StudentPipeline`` on the GPU.  The yardstick is never the new path: the tables of
``rtpe_topk_fused`` and the results of ``parse_lowres`` on the tag map EXPANDED to one plane per joint (what
``eval_student`` builds), PyTorch's own ``F.interpolate`` on the CPU, and the CPU oracle.  Every comparison is
``np.array_equal``; no decode may be empty."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import decode_ref, synth

pytestmark = pytest.mark.gpu

J = 17
DEV = "cuda:0"
COMBOS = [(True, True), (True, False), (False, True), (False, False)]
# (source size, decode size, seeds of the batch's images).  The last three are small outputs (oh + ow <= 128): PyTorch's
# CPU op sums the four products of a sample of channel 16 in another order than those of channels 0..15
SHAPES = [((24, 32), (96, 128), (51, 52, 53)),
          ((12, 16), (48, 64), (53, 51, 52)),
          ((16, 24), (56, 72), (51, 53, 52)),
          ((16, 16), (64, 64), (51, 52, 53))]
SHAPE_IDS = ["%dx%d" % s[1] for s in SHAPES]


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


_MAPS = {}


def _blob_maps(hw, seeds):
    """heat (N,J,h,w) and the shared tag map (N,1,h,w) of a batch, one ``make_decode_maps`` call per image (CPU)"""
    key = (hw, tuple(seeds))
    if key not in _MAPS:
        sets = [synth.make_decode_maps(3, hw[0], hw[1], seed=s, sigma=1.0) for s in seeds]
        heat = torch.from_numpy(np.concatenate([s[0] for s in sets]))
        tag = torch.from_numpy(np.concatenate([s[1][..., 0] for s in sets])).amax(1, keepdim=True)
        _MAPS[key] = (heat, tag)
    return _MAPS[key]


def _det(hw, seeds):
    """det = cat(heat, shared tag): ONE (N, J + 1, h, w) tensor, both arguments of the decode are channel slices of it"""
    heat, tag = _blob_maps(hw, seeds)
    det = torch.cat([heat, tag], 1).contiguous()
    assert tuple(det.shape) == (len(seeds), J + 1) + tuple(hw)
    return det


def _expanded(det):
    """what eval_student hands to parse_lowres: the heat maps and the tag map copied to one plane per joint"""
    return det[:, :J].contiguous(), det[:, J:J + 1].expand(-1, J, -1, -1).contiguous()


def _n_people(people):
    return len(people) if getattr(people, "ndim", 0) == 3 else 0


def _same(got, want):
    gp, gs = got
    wp, ws = want
    assert _n_people(gp) == _n_people(wp)
    assert np.array_equal(np.asarray(gp, np.float32), np.asarray(wp, np.float32))
    assert np.array_equal(np.array(gs, np.float32), np.array(ws, np.float32))


def _not_empty(results, min_people=3):
    """an empty decode cannot pass: people in the batch, rows of (J, 4), and a person with joint 16 present"""
    people = [r[0] for r in results if _n_people(r[0])]
    assert sum(len(p) for p in people) >= min_people
    for p in people:
        assert p.shape[1:] == (J, 4) and p.dtype == np.float32
    assert any((p[:, 16, 2] > 0).any() for p in people)


def _topk(nat, entry, heat, tag, out_hw, K=30, ksize=5, pad=2):
    """one top-k entry of the ABI called directly -> (val_k, ind_k, tag_k) numpy"""
    L = nat.lib()
    N, _, hh, hw = heat.shape
    th, tw = tag.shape[2:]
    oh, ow = out_hw
    nb = ctypes.c_size_t()
    nat.check(L.rtpe_topk_scratch_bytes(N * J, oh, ow, K, ctypes.byref(nb)))
    scratch = torch.empty(max(nb.value, 8), dtype=torch.uint8, device=DEV)
    val = torch.empty((N, J, K), dtype=torch.float32, device=DEV)
    ind = torch.empty((N, J, K), dtype=torch.int32, device=DEV)
    tg = torch.empty((N, J, K, 1), dtype=torch.float32, device=DEV)
    assert heat.stride(1) == hh * hw and tag.stride(1) == th * tw and heat.stride(3) == 1 and tag.stride(3) == 1
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(heat.device):
        nat.check(getattr(L, entry)(p(heat), hh, hw, heat.stride(0), p(tag), th, tw, tag.stride(0), N, J, oh, ow, K,
                                    ksize, pad, p(val), p(ind), p(tg), p(scratch), scratch.numel(),
                                    nat.stream_ptr(heat.device)))
    torch.cuda.synchronize()
    return val.cpu().numpy(), ind.cpu().numpy(), tg.cpu().numpy()


def _tables_agree(nat, heat_slice, tag_slice, out_hw):
    heat_c = heat_slice.contiguous()
    tag_x = tag_slice.expand(-1, J, -1, -1).contiguous()
    want = _topk(nat, "rtpe_topk_fused", heat_c, tag_x, out_hw)
    got = _topk(nat, "rtpe_topk_fused_shared", heat_slice, tag_slice, out_hw)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert (want[0] > 0.1).sum() >= 3 * 3                         # candidates were found
    return want


# --------------------------------------------------------------------------- #
# 1. tables
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("src,out_hw,seeds", SHAPES, ids=SHAPE_IDS)
def test_shared_topk_tables_equal_those_of_the_expanded_tags(nat, src, out_hw, seeds):
    det = _det(src, seeds)
    d = det.to(DEV)
    val_k, ind_k, tag_k = _tables_agree(nat, d[:, :J], d[:, J:], out_hw)
    if out_hw[0] + out_hw[1] > 128:
        return
    # a small output: the shape must exercise the tap order of the vector's tail, or it proves nothing about it.
    # F.interpolate of the expanded map on the CPU: among joint 16's candidates, a pixel whose tag bits differ
    # between channel 16 (the tail) and channel 0
    up = F.interpolate(det[:, J:].expand(-1, J, -1, -1).contiguous(), out_hw, mode="bilinear", align_corners=True)
    differ = 0
    for n in range(det.shape[0]):
        for k in np.nonzero(val_k[n, 16] > 0.1)[0]:
            y, x = divmod(int(ind_k[n, 16, k]), out_hw[1])
            c16, c0 = up[n, 16, y, x].numpy(), up[n, 0, y, x].numpy()
            assert tag_k[n, 16, k, 0].tobytes() == c16.tobytes()       # ... and the kernel took channel 16's order
            differ += c16.tobytes() != c0.tobytes()
    assert differ >= 1


def test_shared_topk_with_the_tag_map_at_half_the_heat_maps_size(nat):
    heat, _ = _blob_maps((48, 64), (51, 52, 53))
    _, tag = _blob_maps((24, 32), (51, 52, 53))
    _tables_agree(nat, heat.to(DEV), tag.to(DEV), (96, 128))


# --------------------------------------------------------------------------- #
# 2. parse_lowres_shared against parse_lowres on the expanded maps
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("src,out_hw,seeds", SHAPES, ids=SHAPE_IDS)
def test_parse_lowres_shared_equals_parse_lowres_on_the_expanded_maps(nat, src, out_hw, seeds, match_on):
    d = _det(src, seeds).to(DEV)
    heat_c, tag_x = _expanded(d)
    for adjust, refine in COMBOS:
        want = _parser(match_on).parse_lowres(heat_c, tag_x, out_hw, adjust, refine)
        got = _parser(match_on).parse_lowres_shared(d[:, :J], d[:, J:], out_hw, adjust, refine)
        assert len(got) == len(seeds) == len(want)
        for g, w in zip(got, want):
            _same(g, w)
        _not_empty(got)


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("src,out_hw,seeds", SHAPES[:2], ids=SHAPE_IDS[:2])
def test_parse_lowres_shared_with_another_parser_setting(nat, src, out_hw, seeds, match_on):
    """K = 12 and a 7x7 NMS window (pad 3): the run-time-padding instantiation of the tile kernel"""
    d = _det(src, seeds).to(DEV)
    heat_c, tag_x = _expanded(d)
    want = _parser(match_on, 12, 7, 3).parse_lowres(heat_c, tag_x, out_hw)
    got = _parser(match_on, 12, 7, 3).parse_lowres_shared(d[:, :J], d[:, J:], out_hw)
    for g, w in zip(got, want):
        _same(g, w)
    _not_empty(got)


def test_parse_lowres_shared_takes_a_three_dimensional_tag_and_leaves_the_state(nat):
    d = _det(*SHAPES[0][::2]).to(DEV)
    p = _parser()
    st = p.lowres_topk_shared(d[:, :J], d[:, J], SHAPES[0][1])
    assert st["refine"][0] == "rtpe_adjust_refine_fused_shared_topk" and st["refine"][2] is True and st["D"] == 1
    assert st["refined"].data_ptr() == d.data_ptr() and st["tags"].data_ptr() == d[:, J:].data_ptr()   # no copies
    p.lowres_match(st)
    got = p.lowres_finish(st)
    want = _parser().parse_lowres(*_expanded(d), SHAPES[0][1])
    for g, w in zip(got, want):
        _same(g, w)
    _not_empty(got)


@pytest.mark.parametrize("src,out_hw,seeds", [SHAPES[0], SHAPES[1]], ids=SHAPE_IDS[:2])
def test_parse_lowres_shared_equals_the_cpu_oracle(nat, src, out_hw, seeds):
    """upsample the expanded maps with the stock CPU op, then the oracle's parse, image by image"""
    det = _det(src, seeds)
    got = _parser().parse_lowres_shared(det.to(DEV)[:, :J], det.to(DEV)[:, J:], out_hw)
    heat_c, tag_x = _expanded(det)
    for n in range(det.shape[0]):
        hms = decode_ref.upsample_bilinear(heat_c[n:n + 1], *out_hw)
        aes = decode_ref.upsample_bilinear(tag_x[n:n + 1], *out_hw)
        want, wsc = decode_ref.HeatmapParserRef().parse(hms, aes.unsqueeze(-1))
        assert 3 <= _n_people(want[0]) <= 6
        _same(got[n], (want[0], wsc))
    _not_empty(got)


# --------------------------------------------------------------------------- #
# 3. / 4. StudentPipeline with a stand-in module
# --------------------------------------------------------------------------- #
class _StandIn(torch.nn.Module):
    """returns prepared (att, det) tensors in call order (fresh tensors: the decode reads them on another stream)"""

    def __init__(self, dets):
        super().__init__()
        self.dets, self.calls = dets, 0

    def forward(self, x, alt=None):
        det = self.dets[self.calls % len(self.dets)].clone()
        self.calls += 1
        return det[:, :1].sigmoid(), det


# five batches of 4 images, at two source sizes
STREAM_SRC = [(24, 32), (12, 16), (24, 32), (12, 16), (24, 32)]
STREAM_HW = [(96, 128), (48, 64), (96, 128), (48, 64), (96, 128)]


@pytest.fixture(scope="module")
def stream_case(nat):
    dets = [_det(src, (51 + k, 52, 53, 50 - k)).to(DEV) for k, src in enumerate(STREAM_SRC)]
    xs = [torch.zeros((4, 3, hw[0], hw[1]), device=DEV) for hw in STREAM_HW]
    want = [_parser().parse_lowres_shared(d[:, :J], d[:, J:], hw) for d, hw in zip(dets, STREAM_HW)]
    for w in want:
        _not_empty(w)
    return dets, xs, want


def test_student_pipeline_call_returns_every_image_of_the_batch(nat, stream_case):
    from rtpe.engine import StudentPipeline
    dets, xs, want = stream_case
    pipe = StudentPipeline(_StandIn(dets), _parser(), DEV)
    for k in (0, 1):
        got = pipe(xs[k])                                           # out_hw defaults to the input size
        assert len(got) == 4
        for g, w in zip(got, want[k]):
            _same(g, w)
    assert pipe.model.calls == 2


@pytest.mark.parametrize("match_on", ["host", "device"])
@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("decode_stream", ["side", "same"])
def test_student_pipeline_stream_equals_call(nat, stream_case, decode_stream, in_flight, match_on):
    from rtpe.engine import StudentPipeline
    dets, xs, want = stream_case
    pipe = StudentPipeline(_StandIn(dets), _parser(), DEV, match_on=match_on)
    assert pipe.parser.match_on == match_on
    asked = []

    def out_hw(k):
        asked.append(k)
        return STREAM_HW[k]
    got = list(pipe.stream(iter(xs), out_hw=out_hw, decode_stream=decode_stream, in_flight=in_flight))
    assert asked == [0, 1, 2, 3, 4] and len(got) == 5
    for k in range(5):                                              # in order
        assert len(got[k]) == 4
        for g, w in zip(got[k], want[k]):
            _same(g, w)


def test_student_pipeline_stream_stopped_early_leaves_the_stream_synchronised(nat, stream_case):
    from rtpe.engine import StudentPipeline
    dets, xs, want = stream_case
    pipe = StudentPipeline(_StandIn(dets), _parser(), DEV)
    gen = pipe.stream(iter(xs), out_hw=lambda k: STREAM_HW[k], in_flight=2)
    first = next(gen)
    gen.close()                                                     # three batches were submitted, one was taken
    for g, w in zip(first, want[0]):
        _same(g, w)
    pipe.model.calls = 0
    again = pipe(xs[0])                                             # on the main stream, right behind the closed loop
    for g, w in zip(again, want[0]):
        _same(g, w)


# --------------------------------------------------------------------------- #
# 5. the real students: plumbing, workspace slots, engine variants
# --------------------------------------------------------------------------- #
def _seeded(cls, shapes_file, seed, golden_dir, *ctor):
    shapes = json.load(open(os.path.join(golden_dir, shapes_file)))["shapes"]
    sd = synth.make_state_dict({k: tuple(v) for k, v in shapes.items()}, seed, "W1")
    stu = cls(None, "cpu", *ctor).eval()
    stu.load_state_dict(sd, strict=True)
    return stu.to(DEV)


def _alone(model, parser, x, hw, **kw):
    """the batch forwarded on its own (workspace slot 0, the caller's stream), decoded as eval_student does it - but
    every image"""
    with torch.no_grad():
        att, det = model(x, **kw)
    assert det.shape == (x.shape[0], J + 1, x.shape[2] // 4, x.shape[3] // 4) and att.shape[1] == 1
    return parser.parse_lowres(*_expanded(det.float()), hw)


def test_student_pipeline_streams_the_attention_student(nat, golden_dir):
    from rtpe.engine import StudentPipeline
    from rtpe.students import AttentionStudent
    stu = _seeded(AttentionStudent, "student_shapes.json", 3, golden_dir, 100, 17, 1, True, None, False)
    xs = [synth.make_images(4, 96, 128, seed=20 + k).to(DEV) for k in range(4)]
    want = [_alone(stu, _parser(), x, (96, 128)) for x in xs]
    got = list(StudentPipeline(stu, _parser(), DEV).stream(iter(xs), in_flight=2))
    assert len(got) == 4
    for k in range(4):
        assert len(got[k]) == 4 == len(want[k])
        for g, w in zip(got[k], want[k]):
            _same(g, w)


def test_student_pipeline_streams_the_steps_student_and_its_divisor_variant(nat, golden_dir):
    from rtpe.engine import StudentPipeline
    from rtpe.students import AttentionStudentSteps
    stu = _seeded(AttentionStudentSteps, "student_steps_shapes.json", 4, golden_dir, 48, 17, 1, True, None, False)
    gen = torch.Generator().manual_seed(31)
    batches = [(synth.make_images(2, 96, 128, seed=40 + k).to(DEV),
                (torch.rand(2, 3, 96, 128, generator=gen) * 100.0).to(DEV)) for k in range(4)]
    pipe = StudentPipeline(stu, _parser(), DEV)
    with pytest.raises(NotImplementedError):
        pipe(batches[0][0])                                         # "ATM alt is expected"
    want = [_alone(stu, _parser(), x, (96, 128), alt=alt) for x, alt in batches]
    got = list(pipe.stream(iter(batches), in_flight=2))
    call = pipe(batches[1][0], alt=batches[1][1])
    # another program of the same module (one executor per att_divisor), through on_forward
    want_div = [_alone(stu, _parser(), x, (96, 128), alt=alt, att_divisor=20.0) for x, alt in batches]
    got_div = list(pipe.stream(iter(batches), in_flight=2,
                               on_forward=lambda k, b: stu(b[0], alt=b[1], att_divisor=20.0)))
    assert len(got) == 4 == len(got_div)
    for k in range(4):
        assert len(got[k]) == 2 == len(got_div[k])
        for g, w in zip(got[k], want[k]):
            _same(g, w)
        for g, w in zip(got_div[k], want_div[k]):
            _same(g, w)
    for g, w in zip(call, want[1]):
        _same(g, w)
