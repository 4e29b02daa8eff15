"""One forward over images of different sizes for AttentionStudentSteps (include/rtpe_hip_mixed_aux.h), on an MI355X
(run with -m gpu).

Per op (tests 1xx): small fp32 ``any_size`` programs with a second input.  Each program runs once on a mixed batch - the
three images of ``M.OP_SIZES`` and their ``alt`` images, in two canvases that are NaN outside every image - through
``rtpe_hrnet_forward_mixed_aux``, with both canvases, both outputs and the workspace between guard bands; and once per
image alone through ``rtpe_hrnet_forward_aux``.  Image n's region of either output must hold the bits of the image alone,
everything outside the regions must be 0.0.  No tolerance anywhere.  Two canvases: 64 x 47, where every image reaches one
canvas edge, and 72 x 80, where none does and a whole tile row and column lie outside every image.

Whole network (2xx, the seeded steps48 of student_steps_shapes.json), ``StudentPipeline`` (3xx), the schedule (4xx) and
the refusals of the C side (5xx) below."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import test_steps_mixed_host as H
import test_student_mixed_gpu as G
import test_student_mixed_host as M
import test_student_sizes_host as S
from oracle import exact, schedule, synth
from test_student_ops_gpu import _ws_guarded
from test_student_pipeline_gpu import _det, _n_people, _parser
from test_student_pipeline_gpu import _same as _same_people

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


@pytest.fixture(autouse=True)
def default_launch_shapes(monkeypatch):
    """the forwards of an image alone at multiples of 32 run on default launch shapes too (test 204 tunes): every launch
    shape gives the same bits, and tuning every small shape of this file would take longer than its tests"""
    monkeypatch.setenv("RTPE_AUTOTUNE", "0")


# --------------------------------------------------------------------------- #
# programs and the two runs
# --------------------------------------------------------------------------- #
def _engine(prog):
    from rtpe.third_party.pose_higher_hrnet import Engine
    p = prog.b.finish()
    assert p.any_size is True and p.has_aux is True
    return Engine(p, 0)


def _alts(sizes, g):
    """the second input: values of a LAB image's span, no relation to the first"""
    return [torch.rand(3, h, w, generator=g) * 100 - 30 for h, w in sizes]


def _forward_mixed_aux_raw(nat, eng, shapes, canvas, alt, sizes, expect_error=False, null_aux=False):
    """rtpe_hrnet_forward_mixed_aux on guarded buffers -> the two output canvases (numpy), or the return code"""
    L = nat.lib()
    N, _, Hc, Wc = canvas.shape
    xg = exact.guarded(canvas.contiguous(), exact.IN_SENTINEL)
    ag = exact.guarded(alt.contiguous(), exact.IN_SENTINEL)
    outs = [exact.guarded_out((N, s_[0], nat.extent(Hc, s_[1]), nat.extent(Wc, s_[1])), torch.float32) for s_ in shapes]
    need = ctypes.c_size_t(1 << 20)
    rc_ws = L.rtpe_hrnet_mixed_workspace_bytes(eng._h, N, Hc, Wc, ctypes.byref(need))
    assert expect_error or rc_ws == 0
    wg = _ws_guarded(max(need.value, 256))
    n_ints = ctypes.c_int32()
    nat.check(L.rtpe_mixed_table_ints(N, ctypes.byref(n_ints)))
    table = G._pinned(n_ints.value)
    flat = (ctypes.c_int32 * (2 * N))(*[v for hw in sizes for v in hw])
    rc = L.rtpe_hrnet_forward_mixed_aux(eng._h, xg.t.data_ptr(), nat.RTPE_DTYPE_F32, None if null_aux else ag.t.data_ptr(), N, Hc,
                                        Wc, flat, table.data_ptr(), table.numel(), outs[0].t.data_ptr(), outs[1].t.data_ptr(),
                                        nat.RTPE_DTYPE_F32, wg.t.data_ptr(), wg.t.numel() * 4, nat.stream_ptr(torch.device(DEV)), 0)
    torch.cuda.synchronize()
    assert exact.guards_intact(xg, ag, outs[0], outs[1], wg), "a guard band was overwritten"
    if expect_error:
        for o in outs:                               # refused before the first launch: nothing was written
            assert rc == 0 or bool((o.t.view(torch.int32) == o.bits).all())
        assert rc == 0 or bool((wg.t == wg.bits).all())
        return rc
    nat.check(rc)
    return [o.t.cpu().numpy() for o in outs]


def _forward_alone_aux_raw(nat, eng, shapes, x, alt):
    """rtpe_hrnet_forward_aux on one image (1, 3, h, w) and its alt, guarded the same way"""
    L = nat.lib()
    _, _, Hh, Ww = x.shape
    xg = exact.guarded(x.contiguous(), exact.IN_SENTINEL)
    ag = exact.guarded(alt.contiguous(), exact.IN_SENTINEL)
    outs = [exact.guarded_out((1, s_[0], nat.extent(Hh, s_[1]), nat.extent(Ww, s_[1])), torch.float32) for s_ in shapes]
    need = ctypes.c_size_t()
    nat.check(L.rtpe_hrnet_workspace_bytes(eng._h, 1, Hh, Ww, ctypes.byref(need)))
    wg = _ws_guarded(max(need.value, 256))
    nat.check(L.rtpe_hrnet_forward_aux(eng._h, xg.t.data_ptr(), nat.RTPE_DTYPE_F32, ag.t.data_ptr(), 1, Hh, Ww, outs[0].t.data_ptr(),
                                       outs[1].t.data_ptr(), nat.RTPE_DTYPE_F32, wg.t.data_ptr(), wg.t.numel() * 4,
                                       nat.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert exact.guards_intact(xg, ag, outs[0], outs[1], wg), "a guard band was overwritten"
    return [o.t.cpu().numpy() for o in outs]


def _mixed_vs_alone(nat, prog, canvas_hw, g, what, sizes=M.OP_SIZES):
    eng = _engine(prog)
    images, alts = G._images(sizes, g), _alts(sizes, g)
    got = _forward_mixed_aux_raw(nat, eng, prog.shapes, G._nan_canvas(images, canvas_hw), G._nan_canvas(alts, canvas_hw), sizes)
    alone = [_forward_alone_aux_raw(nat, eng, prog.shapes, im[None], al[None]) for im, al in zip(images, alts)]
    for a in alone:                                 # the data reach the outputs: a mask that zeroes too much would show
        assert all(float(np.abs(o).max()) > 0 for o in a), what
    return G._check_regions(nat, got, alone, prog.shapes, sizes, "%s in a %d x %d canvas" % ((what,) + tuple(canvas_hw)))


def _select(channels, first, count):
    """a 1x1 conv that copies channels [first, first + count): the output holds the selected values themselves"""
    conv = nn.Conv2d(channels, count, 1, bias=True)
    with torch.no_grad():
        conv.weight.zero_(); conv.bias.zero_()
        for o in range(count):
            conv.weight[o, first + o, 0, 0] = 1.0
    return conv


def _c5(g, cin, cout):
    """a 5x5 stride-2 conv with padding 2, BatchNorm and (at the call) ReLU: the convs of ``alt_img_stem``"""
    return G._conv(g, cin, cout, 5, 2)


def _cat1(nat, p, g, P):
    """[conv (P) | alt at 1/4 (3) | 0]: a conv writing channels [0, P) with cout_store next to the resized second input"""
    b = p.b
    t1 = b.stem(*G._conv(g, 3, 64, 3, 2))
    t2 = b.conv(t1, *G._conv(g, 64, 16, 3, 2), relu=True)                   # 1/4
    cat1 = b.new_tensor(P + 4, 2)
    b.conv(t2, *G._conv(g, 16, P, 3, 1), relu=True, out=(cat1, 0), cout_store=P)
    alt = b.aux_input()
    b.resize(alt, cat1, P, 4)
    return t1, alt, cat1


def _dma_both(nat, run):
    for dma in (1, 0):                                                      # LDS-DMA staging and the register form
        nat.check(nat.lib().rtpe_set_option(b"tile_dma", dma))
        try:
            run(dma)
        finally:
            nat.check(nat.lib().rtpe_set_option(b"tile_dma", 1))


# --------------------------------------------------------------------------- #
# 1xx. per op
# --------------------------------------------------------------------------- #
@G.CANVAS
def test_101_aux_pack_and_resize_next_to_a_slice_conv(nat, canvas_hw):
    """the resize's own arithmetic per image: 33 -> 9 rows and 47 -> 12 columns (scales 3.667 and 3.917, no float32
    numbers: a scale rounded otherwise on the device moves the weights), 64 -> 16 and 32 -> 8 (scale 4); clamped at the
    image's last row, not the canvas' (NaN).  Output 0 copies the four resized channels and the four conv channels before
    them, output 1 is a 3x3 conv over all of them"""
    g = G._gen(1101)
    p = G.Prog(True)
    P = 8
    _, _, cat1 = _cat1(nat, p, g, P)
    p.b.conv(cat1, _select(P + 4, 4, 8), None, out_flag=nat.F_OUT_PREDS, nhwc=False)
    p.shapes[0] = (8, 2)
    p.head(nat, cat1, 4, 1, g, k=3)
    _mixed_vs_alone(nat, p, canvas_hw, g, "aux pack + resize into channels [8, 12)")


@G.CANVAS
def test_102_5x5_stride_2_fp32_conv_from_the_4_channel_second_input(nat, canvas_hw):
    """conv 4 -> 50, BN, ReLU at level 0 -> 1: 25-tap table, pad 2, one 16-channel chunk.  The border taps of an image's
    last rows and columns lie inside the canvas and outside the image: zero padding, not the canvas' NaN"""
    def run(dma):
        g = G._gen(1102)
        p = G.Prog(True)
        alt = p.b.aux_input()
        u = p.b.conv(alt, *_c5(g, 3, 50), relu=True)
        assert p.b.tensors[u][:2] == [56, 1]
        p.head(nat, u, 8, 0, g)
        p.head(nat, u, 4, 1, g, k=3)
        _mixed_vs_alone(nat, p, canvas_hw, g, "5x5 s2 conv 4 -> 50 tile_dma=%d" % dma)
    _dma_both(nat, run)


@G.CANVAS
def test_103_5x5_stride_2_conv_50_to_48_into_a_slice_at_offset_52(nat, canvas_hw):
    """level 1 -> 2, two 32-channel chunks of a 56-channel row, stored with cout_store into channels [52, 100) of a
    100-channel tensor whose channels [0, 52) another conv writes"""
    def run(dma):
        g = G._gen(1103)
        p = G.Prog(True)
        b = p.b
        P = 48
        t1 = b.stem(*G._conv(g, 3, 64, 3, 2))
        cat2 = b.new_tensor(2 * P + 4, 2)
        b.conv(t1, *G._conv(g, 64, P + 4, 3, 2), relu=True, out=(cat2, 0), cout_store=P + 4)
        alt = b.aux_input()
        u = b.conv(alt, *_c5(g, 3, 50), relu=True)
        b.conv(u, *_c5(g, 50, P), relu=True, out=(cat2, P + 4), cout_store=P)
        b.conv(cat2, _select(2 * P + 4, P, 16), None, out_flag=nat.F_OUT_PREDS, nhwc=False)       # both sides of the seam
        p.shapes[0] = (16, 2)
        p.head(nat, cat2, 4, 1, g, k=3)
        _mixed_vs_alone(nat, p, canvas_hw, g, "5x5 s2 conv 50 -> 48 into a slice tile_dma=%d" % dma)
    _dma_both(nat, run)


@G.CANVAS
@pytest.mark.parametrize("div", [None, 20.0], ids=["no_divisor", "div20"])
def test_104_gate_mul_both_outputs(nat, canvas_hw, div):
    """gate_mul runs over the whole canvas: its sigmoid map (output 0) is zeroed outside the regions behind the last op,
    its product (read by a 3x3 conv, output 1) is masked by the reader"""
    g = G._gen(1104, 0 if div is None else 1)
    p = G.Prog(True)
    b = p.b
    P = 8
    _, _, cat1 = _cat1(nat, p, g, P)
    logits = b.conv(cat1, G._conv(g, P + 4, 1, 3, bn=False)[0], None)
    cat2 = b.new_tensor(P + 4, 2)
    b.gate_mul(logits, cat1, cat2, P + 4, div, out_flag=nat.F_OUT_PREDS)
    p.shapes[0] = (1, 2)
    p.head(nat, cat2, 8, 1, g, k=3)
    _mixed_vs_alone(nat, p, canvas_hw, g, "gate_mul divisor %s" % div)


@G.CANVAS
def test_105_col_map_conv_over_the_100_channel_tensor_with_its_hole(nat, canvas_hw):
    """``steps[0]``'s convs: 99 logical input channels at the physical channels [0, 51) and [52, 100) of ``cat2``, channel
    51 the hole (zero weights; inside an image an exact zero, outside whatever the workspace holds)"""
    g = G._gen(1105)
    p = G.Prog(True)
    b = p.b
    P = 48
    t1 = b.stem(*G._conv(g, 3, 64, 3, 2))
    cat2 = b.new_tensor(2 * P + 4, 2)
    b.conv(t1, *G._conv(g, 64, P + 3, 3, 2), relu=True, out=(cat2, 0), cout_store=P + 4)       # (channel 51: the zero pad)
    alt = b.aux_input()
    u = b.conv(alt, *_c5(g, 3, 50), relu=True)
    b.conv(u, *_c5(g, 50, P), relu=True, out=(cat2, P + 4), cout_store=P)
    col_map = list(range(P + 3)) + list(range(P + 4, 2 * P + 4))
    conv, bn = G._conv(g, 2 * P + 3, 16, 3)
    w = torch.zeros(16, 2 * P + 4, 3, 3)
    w[:, col_map] = conv.weight.detach()
    t = b.conv(cat2, conv, bn, relu=True, weight=w)
    p.head(nat, t, 8, 0, g)
    p.head(nat, t, 4, 1, g, k=3)
    _mixed_vs_alone(nat, p, canvas_hw, g, "col_map 3x3 conv over 100 channels")


# --------------------------------------------------------------------------- #
# 2xx. whole network
# --------------------------------------------------------------------------- #
_STEPS = {}
DIVS = (None, 20.0)


def _steps48(golden_dir, fresh=False):
    from rtpe.students import AttentionStudentSteps
    if fresh or "stu" not in _STEPS:
        stu = AttentionStudentSteps(None, "cpu", 48, 17, 1, True, None, False).eval()
        stu.load_state_dict(S.student_sd(golden_dir, "steps"), strict=True)
        if fresh:
            return stu.to(DEV)
        _STEPS["stu"] = stu.to(DEV)
    return _STEPS["stu"]


def _net_pairs():
    """[(x_n, alt_n)] of the whole-network batch: the fixture's two cases first, drawn as the fixture draws them"""
    if "pairs" not in _STEPS:
        _STEPS["pairs"] = [(synth.make_images(1, h, w, seed=s)[0].to(DEV), S.steps_alt(1, h, w, sa)[0].to(DEV))
                           for (h, w), (s, sa) in zip(H.NET_SIZES, H.NET_SEEDS)]
    return _STEPS["pairs"]


def _canvases(pairs, canvas_hw=None):
    xc, sizes = G._canvas([x for x, _ in pairs], canvas_hw)
    ac, sizes_a = G._canvas([a for _, a in pairs], tuple(xc.shape[2:]))
    assert sizes == sizes_a and ac.shape == xc.shape
    return xc, ac, sizes


@pytest.fixture(scope="module")
def net_alone(nat, golden_dir):
    """``stu(x_n[None], alt=alt_n[None], att_divisor=div)`` for every image of the batch and both divisors: computed once"""
    stu = _steps48(golden_dir)
    prev = os.environ.get("RTPE_AUTOTUNE")
    os.environ["RTPE_AUTOTUNE"] = "0"             # (module scope: the function-scoped fixture above is not in force yet)
    try:
        with torch.no_grad():
            return {div: [tuple(t.clone() for t in stu(x[None], alt=a[None], att_divisor=div)) for x, a in _net_pairs()]
                    for div in DIVS}
    finally:
        if prev is None:
            del os.environ["RTPE_AUTOTUNE"]
        else:
            os.environ["RTPE_AUTOTUNE"] = prev


@pytest.mark.parametrize("div", DIVS, ids=["no_divisor", "div20"])
def test_201_forward_mixed_gives_every_image_the_bits_of_its_own_forward(nat, golden_dir, net_alone, div):
    from rtpe.students import unpack_mixed
    stu = _steps48(golden_dir)
    pairs = _net_pairs()
    xc, ac, sizes = _canvases(pairs)
    assert sizes == M.NET_SIZES and xc.shape == (4, 3, 100, 140) and bool(torch.isnan(xc).any()) and bool(torch.isnan(ac).any())
    with torch.no_grad():
        att, det = stu.forward_mixed(xc, sizes, alt=ac, att_divisor=div)
    assert att.shape == (4, 1, 25, 35) and det.shape == (4, 18, 25, 35) and att.dtype == det.dtype == torch.float32
    outside_a, outside_d = att.clone(), det.clone()
    parts = unpack_mixed(att, det, sizes)
    for n, ((a, d), (wa, wd)) in enumerate(zip(parts, net_alone[div])):
        assert torch.equal(a, wa[0]) and torch.equal(d, wd[0]), "image %d (%s)" % (n, sizes[n])
        assert float(d.abs().max()) > 0
        outside_a[n, :, :a.shape[1], :a.shape[2]] = 0
        outside_d[n, :, :d.shape[1], :d.shape[2]] = 0
    assert bool((outside_a == 0).all()) and bool((outside_d == 0).all())              # (NaN == 0 is False)
    # the reference's CPU outputs: image 0 is the fixture's 33 x 47 case (no divisor), image 1 its 100 x 140 case (20.0)
    n, case = (0, S.STEPS_CASES[0]) if div is None else (1, S.STEPS_CASES[1])
    assert case[6] == div and (case[2], case[3]) == sizes[n] and (case[4], case[5]) == H.NET_SEEDS[n]
    g = np.load(os.path.join(golden_dir, "student_sizes.npz"))
    S.within((parts[n][0][None].cpu().numpy(), parts[n][1][None].cpu().numpy()), S.fixture_case(g, "steps", case[0]),
             "steps forward_mixed image %d vs reference steps_%s" % (n, case[0]))
    # the same images in reversed order, and in a canvas 32 larger on both sides: the same bits
    xr, ar, sizes_r = _canvases(pairs[::-1])
    xb, ab, sizes_b = _canvases(pairs, (132, 172))
    with torch.no_grad():
        att_r, det_r = stu.forward_mixed(xr, sizes_r, alt=ar, att_divisor=div)
        att_b, det_b = stu.forward_mixed(xb, sizes_b, alt=ab, att_divisor=div)
    assert att_b.shape == (4, 1, 33, 43)
    for n, (a, d) in enumerate(parts):
        a_r, d_r = unpack_mixed(att_r, det_r, sizes_r)[len(pairs) - 1 - n]
        a_b, d_b = unpack_mixed(att_b, det_b, sizes_b)[n]
        assert torch.equal(a_r, a) and torch.equal(d_r, d) and torch.equal(a_b, a) and torch.equal(d_b, d), n
    assert bool((att_b[:, :, 25:] == 0).all()) and bool((det_b[:, :, :, 35:] == 0).all())


def test_204_two_64x96_images_equal_the_tuned_forward_of_the_pair(nat, golden_dir, monkeypatch):
    """a mixed batch of equal multiple-of-32 images runs the general kernels, ``stu(x, alt=alt)`` of the pair the tuned
    fast ones: the same bits"""
    monkeypatch.delenv("RTPE_AUTOTUNE")
    stu = _steps48(golden_dir)
    x = synth.make_images(2, 64, 96, seed=141).to(DEV)
    alt = S.steps_alt(2, 64, 96, 142).to(DEV)
    with torch.no_grad():
        want = [t.clone() for t in stu(x, alt=alt)]
        att, det = stu.forward_mixed(x, [(64, 96), (64, 96)], alt=alt)
    assert torch.equal(att, want[0]) and torch.equal(det, want[1]) and float(det.abs().max()) > 0


def test_205_a_plain_64x64_forward_after_a_mixed_one_keeps_its_bits(nat, golden_dir):
    """neither the workspace cache nor the tuner carries anything over from a mixed batch"""
    x = synth.make_images(1, 64, 64, seed=99).to(DEV)
    alt = S.steps_alt(1, 64, 64, 98).to(DEV)
    with torch.no_grad():
        want = [t.clone() for t in _steps48(golden_dir, fresh=True)(x, alt=alt)]
    stu = _steps48(golden_dir, fresh=True)
    xc, ac, sizes = _canvases(_net_pairs()[2:])
    assert xc.shape == (2, 3, 96, 96)
    with torch.no_grad():
        stu.forward_mixed(xc, sizes, alt=ac)
        assert not stu._engine(x.device, ("att_divisor", None))._tuned          # a canvas of multiples of 32 is not tuned
        got = stu(x, alt=alt)
        stu.forward_mixed(xc, sizes, alt=ac)
        again = stu(x, alt=alt)
    for a, b_, c in zip(got, want, again):
        assert torch.equal(a, b_) and torch.equal(c, b_)


# --------------------------------------------------------------------------- #
# 3xx. StudentPipeline
# --------------------------------------------------------------------------- #
class _BlobSteps(torch.nn.Module):
    """runs the real Steps student (so that both forwards take the sizes and the second input) and hands out prepared
    blob-bearing det maps instead of its own: seeded networks find no people"""

    def __init__(self, stu, dets):
        super().__init__()
        self.stu, self.dets = stu, dets          # {(h, w): det (1, J + 1, ceil(h/4), ceil(w/4))}
        self.mixed_calls = 0

    def forward(self, x, out_hw=None, alt=None):
        att, det = self.stu(x, alt=alt)
        want = self.dets[tuple(x.shape[2:])]
        assert x.shape[0] == 1 and det.shape == want.shape
        return att, want.clone()

    def forward_mixed(self, canvas, sizes, alt=None):
        att, det = self.stu.forward_mixed(canvas, sizes, alt=alt)
        self.mixed_calls += 1
        det = det.clone()
        for n, hw in enumerate(sizes):
            d = self.dets[tuple(hw)]
            det[n, :, :d.shape[2], :d.shape[3]] = d[0]
        return att, det


PIPE_SIZES = [(100, 140), (64, 96), (96, 128)]


def _pipe_data(golden_dir, match_on):
    from rtpe.engine import StudentPipeline
    dets = {hw: _det((-(-hw[0] // 4), -(-hw[1] // 4)), (51 + i,)).to(DEV) for i, hw in enumerate(PIPE_SIZES)}
    ims = [synth.make_images(1, h, w, seed=70 + i)[0].to(DEV) for i, (h, w) in enumerate(PIPE_SIZES)]
    alts = [S.steps_alt(1, h, w, 80 + i)[0].to(DEV) for i, (h, w) in enumerate(PIPE_SIZES)]
    pipe = StudentPipeline(_BlobSteps(_steps48(golden_dir), dets), _parser(match_on), DEV)
    return pipe, ims, alts


@pytest.mark.parametrize("decode", ["batch", "per_image"])
@pytest.mark.parametrize("match_on", ["host", "device"])
def test_301_call_mixed_equals_the_pipeline_on_every_image_alone(nat, golden_dir, match_on, decode):
    pipe, ims, alts = _pipe_data(golden_dir, match_on)
    got = pipe.call_mixed(ims, alt=alts, decode=decode)
    assert len(got) == 3 and pipe.model.mixed_calls == 1
    for n, (im, al) in enumerate(zip(ims, alts)):
        want = pipe(im[None], alt=al[None])
        assert len(want) == 1 and _n_people(want[0][0]) >= 1, "an empty decode shows nothing"
        _same_people(got[n], want[0])
    with pytest.raises(ValueError, match="needs the second input"):          # before the forward
        pipe.call_mixed(ims)
    assert pipe.model.mixed_calls == 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_302_stream_mixed_over_pairs_of_images_and_alts(nat, golden_dir, in_flight):
    from rtpe.engine import StudentPipeline
    from rtpe.students import pack_mixed
    pipe, ims, alts = _pipe_data(golden_dir, "host")
    orders = [[0, 1, 2], [2, 0], [1, 2, 0]]
    pick = lambda o, src: [src[i] for i in o]
    want = [pipe.call_mixed(pick(o, ims), alt=pick(o, alts)) for o in orders]
    canvas, sizes = pack_mixed(pick(orders[1], ims), (108, 152))          # one triple, in a canvas larger than its images
    triple = (canvas, sizes, pack_mixed(pick(orders[1], alts), (108, 152))[0])
    batches = [(pick(orders[0], ims), pick(orders[0], alts)), triple, (pick(orders[2], ims), pick(orders[2], alts))]
    got = list(pipe.stream_mixed(iter(batches), in_flight=in_flight))
    assert len(got) == 3
    for k, o in enumerate(orders):
        assert len(got[k]) == len(o)
        for i in range(len(o)):
            _same_people(got[k][i], want[k][i])
            assert _n_people(got[k][i][0]) >= 1
    # what mixed_batches cuts goes straight in, and restore gives the caller's order back
    cut, restore = StudentPipeline.mixed_batches(ims, batch_size=2, alts=alts)
    back = restore(list(pipe.stream_mixed(iter(cut), in_flight=in_flight)))
    for n in range(3):
        _same_people(back[n], want[0][n])
    with pytest.raises(ValueError, match="use call_mixed"):                 # stream() keeps refusing such batches
        next(pipe.stream(iter(batches)))
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- #
# 4xx. the schedule of one Steps mixed forward
# --------------------------------------------------------------------------- #
def test_401_the_trace_of_a_mixed_forward_passes_the_happens_before_check(nat, golden_dir):
    from test_schedule_gpu import check_forward
    stu = _steps48(golden_dir)
    eng = stu._engine(torch.device(DEV), ("att_divisor", None))
    xc, ac, sizes = _canvases(_net_pairs()[:2])
    _, _, trace, st = check_forward(eng, lambda: eng.forward_mixed(xc, sizes, aux=ac), "steps mixed", lanes=False)
    assert trace[-1][0] == schedule.MASK and sum(1 for r in trace if r[0] == schedule.MASK) == 1
    print("steps mixed: %s" % st)


# --------------------------------------------------------------------------- #
# 5xx. refusals of the C side, before the first launch
# --------------------------------------------------------------------------- #
def test_501_c_side_refusals(nat, golden_dir):
    from rtpe.students import AttentionStudent
    from rtpe.third_party.pose_higher_hrnet import Engine
    L = nat.lib()
    g = G._gen(1501)
    p = G.Prog(True)
    _, _, cat1 = _cat1(nat, p, g, 8)
    p.head(nat, cat1, 8, 0, g)
    p.head(nat, cat1, 4, 1, g, k=3)
    eng = _engine(p)
    images, alts = G._images(M.OP_SIZES, g), _alts(M.OP_SIZES, g)
    canvas, alt = G._nan_canvas(images, (64, 47)), G._nan_canvas(alts, (64, 47))
    # a null second input
    assert _forward_mixed_aux_raw(nat, eng, p.shapes, canvas, alt, M.OP_SIZES, expect_error=True, null_aux=True) == -1
    assert "second input is null" in L.rtpe_last_error_string().decode()
    # bad sizes, as the entry without a second input refuses them
    assert _forward_mixed_aux_raw(nat, eng, p.shapes, canvas, alt, [(31, 47), (47, 33), (64, 32)], expect_error=True) == -1
    assert "at least 32" in L.rtpe_last_error_string().decode()
    # a handle whose program has no second input
    plain = Engine(AttentionStudent(None, "cpu", 48, 17, 1, True, None, False).eval().compile_program(), 0)
    x = torch.zeros(2, 3, 64, 64)
    assert _forward_mixed_aux_raw(nat, plain, [(1, 2), (18, 2)], x, x, [(64, 64), (32, 64)], expect_error=True) == -1
    assert "no second input" in L.rtpe_last_error_string().decode()
    # the entry without a second input keeps refusing a program that has one; the workspace size serves both
    assert G._forward_mixed_raw(nat, eng, p.shapes, canvas, M.OP_SIZES, expect_error=True) == -1
    assert "second input" in L.rtpe_last_error_string().decode()
    # and the accepted call after all of them
    got = _forward_mixed_aux_raw(nat, eng, p.shapes, canvas, alt, M.OP_SIZES)
    assert all(np.isfinite(o).all() for o in got) and float(np.abs(got[1]).max()) > 0
