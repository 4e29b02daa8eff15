"""The students at input sizes that are not multiples of 32, on an MI355X (run with -m gpu).

Per op, exact (tests 1xx below): small programs built with the ``any_size`` property, the method of
tests/test_student_ops_gpu.py and tests/test_conv_exact_gpu.py - integer data on which every sum is exact in any order,
float64 references with the kernels' rounding points, ``array_equal``.  x, the second input, both outputs and the workspace
sit between guard bands; the outputs are preset to a NaN pattern and the workspace to a finite sentinel, so a store beyond
a ragged right or bottom edge and a pixel an op never writes both show.

Whole network (tests 2xx): both students against the reference's CPU outputs at such sizes
(tests/golden/student_sizes.npz) and against the oracle, with the bound of the students' other GPU tests
(``|att - ref| <= 1e-3``, ``|det - ref| <= 1e-3 * max(1, |ref det| max)``: BASELINE's heat-map tolerance); batch
invariance; ``eval_student`` and ``StudentPipeline`` at such sizes, bit-identical to ``parse_lowres`` on the expanded
maps; and a multiple-of-32 forward after a ragged one, bit-identical to the same forward on a fresh module."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_student_ops_host as T
import test_student_sizes_host as S
from oracle import decode_ref, exact, student_ref, synth
from oracle import student_ops as so
from test_conv_exact_gpu import _same
from test_conv_exact_host import SEED, _layer, _ref_layer
from test_student_ops_gpu import Net, _f32np, _se_program, _sigmoid_ok, _ws_guarded
from test_student_pipeline_gpu import _det, _expanded, _n_people, _parser
from test_student_pipeline_gpu import _same as _same_people

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = torch.float64
J = 17


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


def _run(nat, net, N, H, W, x=None, aux=None, expect_error=False, any_size=True):
    """test_student_ops_gpu._run for a program with the any_size property: one forward on guarded x, aux, outputs and
    workspace; the outputs hold ``extent`` pixels per side.  Returns the two outputs (numpy), or the return code"""
    from rtpe.third_party.pose_higher_hrnet import Engine
    net.b.any_size = any_size
    prog = net.b.finish()
    assert prog.any_size is any_size
    eng = Engine(prog, 0)
    L = nat.lib()
    on = ctypes.c_int32(-1)
    nat.check(L.rtpe_hrnet_get_any_size(eng._h, ctypes.byref(on)))
    assert on.value == int(any_size)
    if x is None:
        x = torch.zeros(N, 3, H, W, dtype=torch.float16)
    xg = exact.guarded(x.contiguous(), exact.IN_SENTINEL)
    ag = exact.guarded(aux.float().contiguous(), exact.IN_SENTINEL) if aux is not None else None
    assert bool(getattr(prog, "has_aux", False)) == (aux is not None)
    outs = []
    for s_ in net.shapes:
        shape = (N, s_[0], nat.extent(H, s_[1]), nat.extent(W, s_[1])) if s_ else (1, 1, 1, 64)
        outs.append(exact.guarded_out(shape, torch.float32))
    need = ctypes.c_size_t(1 << 20)
    rc_ws = L.rtpe_hrnet_workspace_bytes(eng._h, N, H, W, ctypes.byref(need))
    assert (rc_ws == 0) == (any_size or not nat.ragged(H, W))
    wg = _ws_guarded(max(need.value, 256))
    st = nat.stream_ptr(torch.device(DEV))
    xdt = nat.RTPE_DTYPE_F16 if x.dtype == torch.float16 else nat.RTPE_DTYPE_F32
    if aux is not None:
        rc = L.rtpe_hrnet_forward_aux(eng._h, xg.t.data_ptr(), xdt, ag.t.data_ptr(), N, H, W, outs[0].t.data_ptr(),
                                      outs[1].t.data_ptr(), nat.RTPE_DTYPE_F32, wg.t.data_ptr(), wg.t.numel() * 4, st)
    else:
        rc = L.rtpe_hrnet_forward_flags(eng._h, xg.t.data_ptr(), xdt, N, H, W, outs[0].t.data_ptr(), outs[1].t.data_ptr(),
                                        nat.RTPE_DTYPE_F32, wg.t.data_ptr(), wg.t.numel() * 4, st, 0)
    torch.cuda.synchronize()
    assert exact.guards_intact(xg, ag, outs[0], outs[1], wg), "a guard band was overwritten"
    if expect_error:
        for o in outs:                               # refused before the first launch: nothing was written
            assert rc == 0 or bool((o.t.view(torch.int32) == o.bits).all())
        return rc
    nat.check(rc)
    return [o.t.cpu().numpy() for o in outs]


def _aux_chain(N, H, W, ds, g, lo=-5, hi=5):
    """a seeded integer second input (N, 3, H, W) and the float64 map behind each of ``ds`` centre-tap stride-2 convs
    (Net.chain): chain[i] holds ceil(H / 2^i) x ceil(W / 2^i) pixels, 8 channels of which 3 are used (chain[0]: 4)"""
    aux = torch.randint(lo, hi + 1, (N, 3, H, W), generator=g).double()
    chain = [so.aux_pack(aux)]
    for i in range(ds):
        chain.append(so.exact_conv(chain[-1], T.sub_weights(chain[-1].shape[1]), None, 2))
        assert chain[-1].shape[2:] == (-(-H // (2 << i)), -(-W // (2 << i)))
        assert torch.equal(chain[-1][:, :3], aux[:, :, ::2 << i, ::2 << i])
    return aux, chain


def _gen(*key):
    return torch.Generator().manual_seed(SEED + 4242 + sum((i + 1) * 131 * int(k) for i, k in enumerate(key)))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


# --------------------------------------------------------------------------- #
# 101. fp16: stem conv1 and stride-2 3x3 convs with odd input sides
# --------------------------------------------------------------------------- #
# (N, H, W): the stem's map, the map behind the 64 -> 64 stride-2 conv = the input of the conv under test, its output:
#   33 x 47: 17 x 24,  9 x 12 (odd x multiple of 4), 5 x 6       34 x 38: 17 x 19,  9 x 10, 5 x 5
#   66 x 70: 33 x 35, 17 x 18 (odd x even),          9 x 9       38 x 42: 19 x 21, 10 x 11, 5 x 6
FP16_SHAPES = [(2, 33, 47), (1, 66, 70), (1, 38, 42), (1, 34, 38)]


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("shape", FP16_SHAPES, ids=lambda s: "n%d_%dx%d" % s)
def test_101_fp16_stem_and_stride2_convs_with_odd_sides_are_exact(nat, shape, relu):
    """stem 3 -> 64 (the VALU kernel), conv 64 -> 64 k3 s2, conv 64 -> 48 k3 s2 (with and without ReLU) and two 1x1 heads
    with bias and fp32 NCHW output whose width is 6, 9 or 5: every conv on the one-workgroup-per-tile kernel.  The last
    output row / column of each stride-2 layer reads one tap beyond its input map: zero, not the next row's first pixel"""
    N, H, W = shape
    g = torch.Generator().manual_seed(SEED + 7 * H + W)
    stem, conv2, conv3 = _layer(3, 64, 3, 2, g), _layer(64, 64, 3, 2, g), _layer(64, 48, 3, 2, g)
    heads = [_layer(48, 34, 1, 1, g, bn=False), _layer(48, 17, 1, 1, g, bn=False)]
    net = Net(f32=False)
    b = net.b
    t = b.stem(stem[0], stem[1])
    t = b.conv(t, conv2[0], conv2[1], relu=True)
    t = b.conv(t, conv3[0], conv3[1], relu=relu)
    b.conv(t, heads[0][0], None, out_flag=nat.F_OUT_PREDS, nhwc=False)
    b.conv(t, heads[1][0], None, out_flag=nat.F_OUT_REFINED, nhwc=False)
    net.shapes = [(34, 3), (17, 3)]
    x = torch.randint(-3, 4, (N, 3, H, W), generator=g).half()
    y = _ref_layer(x.double(), stem, 3, 2, True, True, quantum=1.0)
    assert y.shape[2:] == (nat.extent(H, 1), nat.extent(W, 1))
    y = _ref_layer(y, conv2, 3, 2, True, True, quantum=0.5)
    y = _ref_layer(y, conv3, 3, 2, relu, True, quantum=0.25)
    assert y.shape[2:] == (nat.extent(H, 3), nat.extent(W, 3))
    want = [_ref_layer(y, hd, 1, 1, False, False, quantum=0.125).float().numpy() for hd in heads]
    got = _run(nat, net, N, H, W, x=x)
    what = "fp16 chain n%d %dx%d relu=%s" % (N, H, W, relu)
    _same(got[0], want[0], what + " head 34")
    _same(got[1], want[1], what + " head 17")


# --------------------------------------------------------------------------- #
# 102. fp32: stride-2 3x3 and 5x5 convs with odd input sides
# --------------------------------------------------------------------------- #
# (N, H, W, ds of the input map): 9 x 12, 17 x 18, 10 x 11
F32_S2_SHAPES = [(2, 33, 47, 2), (1, 33, 35, 1), (1, 38, 42, 2)]


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("shape", F32_S2_SHAPES, ids=lambda s: "n%d_%dx%d_ds%d" % s)
def test_102_fp32_stride2_conv_with_odd_sides_is_exact(nat, shape, relu):
    N, H, W, ds = shape
    g = _gen(102, H, W, relu)
    aux, chain = _aux_chain(N, H, W, ds, g)
    C = 16
    w, bias = _ints(g, -1, 1, C, chain[-1].shape[1], 3, 3), _ints(g, -6, 6, C)
    net = Net(f32=True)
    t = net.chain(ds)[-1]
    t = net.b.conv(t, Net._conv(w, bias, 2), None, relu=relu)
    assert net.b.tensors[t][1] == ds + 1
    net.head(t, range(0, 8), 0)
    net.head(t, range(8, C), 1)
    want = so.exact_conv(chain[-1], w, bias, 2, relu)
    assert want.shape[2:] == (nat.extent(H, ds + 1), nat.extent(W, ds + 1)) and (want != 0).double().mean() > 0.3
    got = _run(nat, net, N, H, W, aux=aux)
    what = "fp32 conv k3 s2 of a %d x %d map relu=%s" % (chain[-1].shape[2], chain[-1].shape[3], relu)
    _same(got[0], _f32np(want[:, :8]), what)
    _same(got[1], _f32np(want[:, 8:]), what)


def test_102_fp32_5x5_stride2_conv_at_33x47_is_exact(nat):
    """the first conv of the Steps student's alt stem: 5x5 stride 2 on the packed second input at full resolution"""
    N, H, W = 2, 33, 47
    g = _gen(1025, H, W)
    aux, chain = _aux_chain(N, H, W, 0, g)
    C = 16
    w, bias = _ints(g, -1, 1, C, 4, 5, 5), _ints(g, -6, 6, C)
    net = Net(f32=True)
    t = net.b.conv(net.b.aux_input(), Net._conv(w, bias, 2), None, relu=True)
    net.head(t, range(0, 8), 0)
    net.head(t, range(8, C), 1)
    want = so.exact_conv(chain[0], w, bias, 2, True)
    assert want.shape[2:] == (17, 24)
    got = _run(nat, net, N, H, W, aux=aux)
    _same(got[0], _f32np(want[:, :8]), "fp32 conv k5 s2 at 33 x 47")
    _same(got[1], _f32np(want[:, 8:]), "fp32 conv k5 s2 at 33 x 47")


# --------------------------------------------------------------------------- #
# 103. avgpool
# --------------------------------------------------------------------------- #
# (N, H, W, ds): maps 9 x 12 -> 5 x 6, 5 x 6 -> 3 x 3, 1 x 3 -> 1 x 2, 2 x 1 -> 1 x 1
AVGPOOL_SHAPES = [(2, 33, 47, 2, (9, 12)), (1, 33, 47, 3, (5, 6)), (2, 40, 150, 6, (1, 3)), (3, 100, 40, 6, (2, 1))]


@pytest.mark.parametrize("shape", AVGPOOL_SHAPES, ids=lambda s: "n%d_%dx%d_ds%d" % s[:4])
def test_103_avgpool_of_maps_with_odd_sides_is_exact(nat, shape):
    """ceil(h / 2) x ceil(w / 2) outputs; at the high edge of an odd side the window holds 2 (or, one pixel wide, 1) taps
    per axis and divides by their number"""
    N, H, W, ds, hw = shape
    g = _gen(103, H, W, ds)
    aux, chain = _aux_chain(N, H, W, ds, g, -9, 9)
    assert tuple(chain[-1].shape[2:]) == hw
    C = 16
    w, bias = T.mix_weights(g, C, 8, bias_amp=4)
    net = Net(f32=True)
    t = net.b.avgpool(net.tensor(net.chain(ds)[-1], C, w, bias))
    net.head(t, range(0, 8), 0)
    net.head(t, range(8, C), 1)
    ref = so.avgpool(so.exact_conv(chain[-1], w, bias))
    assert tuple(ref.out.shape[2:]) == (-(-hw[0] // 2), -(-hw[1] // 2))
    got = _run(nat, net, N, H, W, aux=aux)
    what = "avgpool of a %d x %d map (divisors %s)" % (hw + (ref.counts,))
    _same(got[0], _f32np(ref.out[:, :8]), what)
    _same(got[1], _f32np(ref.out[:, 8:]), what)


# --------------------------------------------------------------------------- #
# 104. fuse with up-sampled terms: the nearest-to-size sampler
# --------------------------------------------------------------------------- #
# (N, H, W): terms at 1/16 and 1/8 into the map at 1/4: 3 x 3 and 5 x 6 into 9 x 12; 7 x 9 and 13 x 18 into 25 x 35
FUSE_SHAPES = [(2, 33, 47), (1, 100, 140)]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", FUSE_SHAPES, ids=lambda s: "n%d_%dx%d" % s)
def test_104_fuse_reads_lower_resolution_terms_with_the_nearest_to_size_rule(nat, shape, relu):
    """hi + up(lo at 1/16) + up(mid at 1/8) as F.interpolate(mode="nearest", size=...) on the CPU gives it.  Channel 0 of
    every source map holds a different number in every pixel, so a wrong source index changes the value; the shift
    ``dst >> up`` gives another result for the 4x term"""
    N, H, W = shape
    g = _gen(104, H, W)
    aux = torch.randint(-5, 6, (N, 3, H, W), generator=g).double()
    for ds, base in ((2, 1000), (3, 2000), (4, 3000)):       # plane 0: a pixel's own number at every level of the chain
        h, w = -(-H // (1 << ds)), -(-W // (1 << ds))
        ids = base + torch.arange(h * w, dtype=D).view(h, w)
        aux[:, 0, ::1 << ds, ::1 << ds] = ids + 500 * torch.arange(N, dtype=D).view(N, 1, 1)
    chain = [so.aux_pack(aux)]
    for i in range(4):
        chain.append(so.exact_conv(chain[-1], T.sub_weights(chain[-1].shape[1]), None, 2))
    for ds in (3, 4):
        flat = chain[ds][:, 0].flatten(1)
        assert all(len(set(r.tolist())) == r.numel() for r in flat), "every source pixel distinct"
    C = 8
    ws = []
    for _ in range(3):
        w, bias = T.mix_weights(g, C, 8, bias_amp=3)
        w[0] = 0
        w[0, 0] = 1                                           # channel 0 = plane 0 (+ bias)
        ws.append((w, bias))
    net = Net(f32=True)
    ch = net.chain(4)
    hi, mid, lo = [net.tensor(ch[ds], C, *ws[i]) for i, ds in enumerate((2, 3, 4))]
    out = net.b.fuse([(hi, 0), (lo, 2), (mid, 1)], relu=relu)
    net.head(out, range(0, 4), 0)
    net.head(out, range(4, C), 1)
    r_hi, r_mid, r_lo = [so.exact_conv(chain[ds], *ws[i]) for i, ds in enumerate((2, 3, 4))]
    size = tuple(r_hi.shape[2:])
    assert size == (nat.extent(H, 2), nat.extent(W, 2))
    up = lambda t: F.interpolate(t.float(), size=size, mode="nearest").double()
    want = (r_hi + up(r_lo)) + up(r_mid)                       # integers: every fp32 add is exact
    shifted = (r_hi + r_lo[:, :, (torch.arange(size[0]) >> 2).clamp(max=r_lo.shape[2] - 1)][..., (torch.arange(size[1]) >> 2).clamp(max=r_lo.shape[3] - 1)]) \
        + r_mid[:, :, torch.arange(size[0]) >> 1][..., torch.arange(size[1]) >> 1]
    assert not torch.equal(shifted, want), "this shape cannot tell the shift from the rule"
    if relu:
        want = torch.where(want > 0, want, torch.zeros_like(want))
    got = _run(nat, net, N, H, W, aux=aux)
    what = "fuse %s and %s into %s relu=%s" % (tuple(r_lo.shape[2:]), tuple(r_mid.shape[2:]), size, relu)
    _same(got[0], _f32np(want[:, :4]), what)
    _same(got[1], _f32np(want[:, 4:]), what)


# --------------------------------------------------------------------------- #
# 105. the fp32 head with NCHW output at widths that are no multiples of 4
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", [(2, 100, 140, (25, 35)), (2, 33, 35, (9, 9))], ids=lambda s: "n%d_%dx%d" % s[:3])
def test_105_fp32_nchw_head_at_odd_widths_is_exact(nat, shape):
    """the students' last op: conv 3x3 with bias, fp32, NCHW output only (18 channels), on a 25 x 35 and a 9 x 9 map: no
    16-byte store may run over a row end, every row keeps its own pixels"""
    N, H, W, hw = shape
    g = _gen(105, H, W)
    aux, chain = _aux_chain(N, H, W, 2, g)
    assert tuple(chain[2].shape[2:]) == hw
    w, bias = _ints(g, -1, 1, 18, 8, 3, 3), _ints(g, -6, 6, 18)
    w1, b1 = _ints(g, -1, 1, 1, 8, 3, 3), _ints(g, -6, 6, 1)
    net = Net(f32=True)
    t = net.chain(2)[-1]
    net.b.conv(t, Net._conv(w1, b1, 1), None, out_flag=nat.F_OUT_PREDS, nhwc=False)
    net.b.conv(t, Net._conv(w, bias, 1), None, out_flag=nat.F_OUT_REFINED, nhwc=False)
    net.shapes = [(1, 2), (18, 2)]
    got = _run(nat, net, N, H, W, aux=aux)
    _same(got[0], _f32np(so.exact_conv(chain[2], w1, b1)), "fp32 NCHW head, 1 channel, width %d" % hw[1])
    _same(got[1], _f32np(so.exact_conv(chain[2], w, bias)), "fp32 NCHW head, 18 channels, width %d" % hw[1])


# --------------------------------------------------------------------------- #
# 106. SE gate at a 9 x 12 map
# --------------------------------------------------------------------------- #
T.SE_MAPS.setdefault(108, (36, 48, 2))       # HW = 108: a 36 x 48 input (no multiples of 32), the 9 x 12 map at 1/4


def test_106_se_gate_divides_by_the_true_pixel_count_of_a_9x12_map(nat):
    C, hid, in_ld, zero_cols = T.emitted().se[0]
    d = T.se_data(C, hid, in_ld, zero_cols, 108)
    assert (d.H, d.W, d.ds) == (36, 48, 2) and nat.ragged(d.H, d.W) and tuple(d.x.shape[2:]) == (9, 12)
    net, gl = _se_program(C, hid, in_ld, zero_cols, d.ds, d.wx, d.bx, d.w1, d.b1, d.w2, d.b2, d.w_res, d.b_res, d.w_hdc, d.b_hdc)
    got = _run(nat, net, d.N, d.H, d.W, aux=d.aux)
    what = "se C=%d hid=%d at a 9 x 12 map" % (C, hid)
    rows = got[0][:, :, 0, 0]
    _same(got[0], np.ascontiguousarray(np.broadcast_to(rows[:, :, None, None], got[0].shape)), what + ": one gate per image")
    _sigmoid_ok(rows[:, :C], d.ref.logit, None, what)
    emitted = torch.from_numpy(np.ascontiguousarray(rows)).double()
    _same(got[1], _f32np(so.cam_combine(d.res, d.hdc, emitted)), what + ": combine of the emitted gates")
    # a mean over another pixel count (96 = 8 x 12, 117 = 9 x 13, ...) moves the exact gates: 0.5 where the logit is 0
    ex = so.sigmoid_map(d.ref.logit).exact
    assert ex.any() and np.array_equal(rows[:, :C][ex.numpy()], so.sigmoid_map(d.ref.logit).want.float().numpy()[ex.numpy()])


# --------------------------------------------------------------------------- #
# 107. refusals of the C side, before the first launch
# --------------------------------------------------------------------------- #
def test_107_a_program_without_the_property_and_a_transposed_conv_are_refused(nat):
    import torch.nn as nn
    g = _gen(107)
    aux = torch.randint(-5, 6, (1, 3, 33, 47), generator=g).double()
    net = Net(f32=True)
    net.head(net.chain(2)[-1], range(4), 0)
    rc = _run(nat, net, 1, 33, 47, aux=aux, expect_error=True, any_size=False)
    msg = nat.lib().rtpe_last_error_string().decode()
    assert rc == -1 and "multiples of 32" in msg and "any_size" in msg, (rc, msg)
    # the same program takes a multiple of 32, and with the property the ragged size
    net = Net(f32=True)
    net.head(net.chain(2)[-1], range(4), 0)
    _run(nat, net, 1, 32, 64, aux=torch.zeros(1, 3, 32, 64), any_size=False)
    # sides below 32
    net = Net(f32=True)
    net.head(net.chain(2)[-1], range(4), 0)
    assert _run(nat, net, 1, 31, 47, aux=torch.zeros(1, 3, 31, 47), expect_error=True) == -1
    # an op without a general path at a ragged map
    net = Net(f32=False)
    stem = _layer(3, 64, 3, 2, g)
    t = net.b.stem(stem[0], stem[1])
    dc = nn.ConvTranspose2d(64, 32, 4, 2, 1, bias=False)
    t = net.b.deconv(t, dc, nn.BatchNorm2d(32))
    net.b.conv(t, _layer(32, 17, 1, 1, g, bn=False)[0], None, out_flag=nat.F_OUT_PREDS, nhwc=False)
    net.shapes = [(17, 0), None]
    rc = _run(nat, net, 1, 33, 47, expect_error=True)
    msg = nat.lib().rtpe_last_error_string().decode()
    assert rc == -1 and "transposed conv" in msg, (rc, msg)


# --------------------------------------------------------------------------- #
# 2xx. whole network
# --------------------------------------------------------------------------- #
def _student100(golden_dir):
    from rtpe.students import AttentionStudent
    stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False).eval()
    sd = S.student_sd(golden_dir, "s100")
    stu.load_state_dict(sd, strict=True)
    return stu.to(DEV), sd


def _steps48(golden_dir):
    from rtpe.students import AttentionStudentSteps
    stu = AttentionStudentSteps(None, "cpu", 48, 17, 1, True, None, False).eval()
    sd = S.student_sd(golden_dir, "steps")
    stu.load_state_dict(sd, strict=True)
    return stu.to(DEV), sd


def test_201_attention_student_vs_the_reference_fixture_and_the_oracle(nat, golden_dir):
    g = np.load(os.path.join(golden_dir, "student_sizes.npz"))
    stu, sd = _student100(golden_dir)
    for name, n, h, w, seed in S.S100_CASES:
        x = synth.make_images(n, h, w, seed=seed)
        with torch.no_grad():
            att, det = stu(x.to(DEV))
        assert att.shape == (n, 1, -(-h // 4), -(-w // 4)) and det.shape == (n, 18, -(-h // 4), -(-w // 4))
        assert att.dtype == torch.float32 and det.dtype == torch.float32
        got = (att.cpu().numpy(), det.cpu().numpy())
        full = S.fixture_case(g, "s100", name)
        if full is None:
            S.sampled_within(g, "s100", name, got[0], got[1], "student100 vs reference " + name)
        else:
            S.within(got, full, "student100 vs reference " + name)
        oa, od = student_ref.student_forward(sd, x, half_stem=True)
        S.within(got, (oa.numpy(), od.numpy()), "student100 vs oracle " + name)


def test_202_attention_student_steps_vs_the_reference_fixture_and_the_oracle(nat, golden_dir):
    g = np.load(os.path.join(golden_dir, "student_sizes.npz"))
    stu, sd = _steps48(golden_dir)
    for name, n, h, w, seed, alt_seed, div in S.STEPS_CASES:
        x, alt = synth.make_images(n, h, w, seed=seed), S.steps_alt(n, h, w, alt_seed)
        with torch.no_grad():
            att, det = stu(x.to(DEV), alt=alt.to(DEV)) if div is None else stu(x.to(DEV), alt=alt.to(DEV), att_divisor=div)
        assert att.shape == (n, 1, -(-h // 4), -(-w // 4)) and det.shape == (n, 18, -(-h // 4), -(-w // 4))
        got = (att.cpu().numpy(), det.cpu().numpy())
        S.within(got, S.fixture_case(g, "steps", name), "steps48 vs reference " + name)
        oa, od = student_ref.student_steps_forward(sd, x, alt, div, half_stem=True)
        S.within(got, (oa.numpy(), od.numpy()), "steps48 vs oracle " + name)


def test_203_fp32_stem_student_at_38x50_vs_the_oracle(nat):
    from rtpe.students import AttentionStudent
    stu = AttentionStudent(None, "cpu", 64, 17, 1, False, None, False).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in stu.state_dict().items()}, 5, "W1")
    stu.load_state_dict(sd, strict=True)
    stu = stu.to(DEV)
    x = synth.make_images(2, 38, 50, seed=9)
    oa, od = student_ref.student_forward(sd, x, half_stem=False)
    with torch.no_grad():
        att, det = stu(x.to(DEV))
    assert att.shape == (2, 1, 10, 13)
    S.within((att.cpu().numpy(), det.cpu().numpy()), (oa.numpy(), od.numpy()), "fp32-stem student 38x50 vs oracle")


def test_204_batch_invariance_at_50x70(nat, golden_dir):
    """three images of 50 x 70 give the bits each gives alone (launch shapes depend on the batch size, results must not)"""
    stu, _ = _student100(golden_dir)
    x = synth.make_images(3, 50, 70, seed=21).to(DEV)
    with torch.no_grad():
        att, det = stu(x)
        for i in range(3):
            a1, d1 = stu(x[i:i + 1])
            assert torch.equal(a1[0], att[i]) and torch.equal(d1[0], det[i]), i
    assert att.shape == (3, 1, 13, 18) and float(det.abs().max()) > 0


def test_205_a_multiple_of_32_after_a_ragged_forward_keeps_its_bits(nat, golden_dir):
    """320 x 320 after 100 x 140 on one module equals 320 x 320 on a fresh module bit for bit: neither the workspace cache
    nor the tuner carries anything over from a ragged shape - which is never tuned"""
    x = synth.make_images(1, 320, 320, seed=99).to(DEV)
    xr = synth.make_images(1, 100, 140, seed=102).to(DEV)
    fresh, _ = _student100(golden_dir)
    with torch.no_grad():
        want = [t.clone() for t in fresh(x)]
    stu, _ = _student100(golden_dir)
    with torch.no_grad():
        stu(xr)
        eng = stu._engine(x.device)
        assert (1, 100, 140) not in eng._tuned and all(k[1] % 32 == 0 and k[2] % 32 == 0 for k in eng._tuned)
        n_ints = ctypes.c_int32()
        nat.check(nat.lib().rtpe_hrnet_tuned_ints(eng._h, ctypes.byref(n_ints)))
        buf = (ctypes.c_int32 * n_ints.value)()
        assert nat.lib().rtpe_hrnet_export_tuned(eng._h, 1, 100, 140, buf, n_ints.value) != 0
        assert b"has not been tuned" in nat.lib().rtpe_last_error_string()     # ... on the C side either
        got = stu(x)
        stu(xr)
        again = stu(x)
    for a, b_, c in zip(got, want, again):
        assert torch.equal(a, b_) and torch.equal(c, b_)


# --------------------------------------------------------------------------- #
# 21x. eval_student and StudentPipeline at ragged sizes
# --------------------------------------------------------------------------- #
class _BlobStudent(torch.nn.Module):
    """runs the real student (so that its forward takes the size), checks the shape of what it returns and hands out
    prepared blob-bearing det maps of that shape instead: seeded networks find no people"""

    def __init__(self, stu, dets):
        super().__init__()
        self.stu, self.dets, self.calls = stu, dets, 0

    def forward(self, x, out_hw=None, alt=None):
        att, det = self.stu(x)
        want = self.dets[self.calls % len(self.dets)]
        self.calls += 1
        h, w = -(-x.shape[2] // 4), -(-x.shape[3] // 4)
        assert att.shape == (x.shape[0], 1, h, w) and det.shape == want.shape == (x.shape[0], J + 1, h, w)
        return att, want.clone()


def _oracle_people(det, hw):
    """people of every image of a det batch at decode size hw, by the CPU oracle"""
    heat, tag = _expanded(det.cpu())
    out = []
    for n in range(det.shape[0]):
        hms = decode_ref.upsample_bilinear(heat[n:n + 1], *hw)
        aes = decode_ref.upsample_bilinear(tag[n:n + 1], *hw)
        ans, _ = decode_ref.HeatmapParserRef().parse(hms, aes.unsqueeze(-1))
        out.append(_n_people(ans[0]))
    return out


def test_211_eval_student_takes_native_size_images(nat, golden_dir):
    """a two-item loader of a 33 x 47 and a 100 x 140 image (batch 1, out_hw = img.shape[2:], as the reference's minival):
    no error, and the results equal ``parse_lowres`` on the expanded maps"""
    from rtpe.engine import eval_student
    stu, _ = _student100(golden_dir)
    sizes = [(33, 47), (100, 140)]
    dets = [_det((-(-h // 4), -(-w // 4)), (51 + i,)).to(DEV) for i, (h, w) in enumerate(sizes)]
    seen = {}

    class _Data:
        def evaluate(self, preds, scores, *a):
            seen["preds"], seen["scores"] = preds, scores
            return {"images": len(preds)}, None

    class _Loader(list):
        dataset = _Data()

    loader = _Loader((i, synth.make_images(1, h, w, seed=30 + i)) for i, (h, w) in enumerate(sizes))
    res = eval_student(_BlobStudent(stu, dets), _parser(), loader, DEV)
    assert res == {"images": 2}
    found = 0
    for i, (d, hw) in enumerate(zip(dets, sizes)):
        want = _parser().parse_lowres(*_expanded(d), hw)[0]
        got_people = seen["preds"][i]
        assert len(got_people) == _n_people(want[0])
        if len(got_people):
            assert np.array_equal(np.stack(got_people), np.asarray(want[0], np.float32))
        assert np.array_equal(np.array(seen["scores"][i], np.float32), np.array(want[1], np.float32))
        found += len(got_people)
    assert _oracle_people(dets[1], sizes[1])[0] >= 1 and found >= 1


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_212_student_pipeline_call_and_stream_at_100x140(nat, golden_dir, match_on):
    """2 x 3 x 100 x 140: the decode size defaults to (100, 140), ``parse_lowres_shared`` maps 25 x 35 to it; per image
    bit-identical to ``parse_lowres(det[:, :J], det[:, J:].expand(...), (100, 140))``; at least one person per image"""
    from rtpe.engine import StudentPipeline
    stu, _ = _student100(golden_dir)
    hw = (100, 140)
    dets = [_det((25, 35), seeds).to(DEV) for seeds in ((51, 52), (53, 51), (52, 53))]
    for d in dets:
        assert all(p >= 1 for p in _oracle_people(d, hw))
    want = [_parser(match_on).parse_lowres(*_expanded(d), hw) for d in dets]
    for w_ in want:
        assert len(w_) == 2 and all(_n_people(r[0]) >= 1 for r in w_)
    xs = [synth.make_images(2, 100, 140, seed=40 + k).to(DEV) for k in range(3)]
    model = _BlobStudent(stu, dets)
    pipe = StudentPipeline(model, _parser(match_on), DEV)
    for k in range(2):
        got = pipe(xs[k])
        assert len(got) == 2
        for g_, w_ in zip(got, want[k]):
            _same_people(g_, w_)
    model.calls = 0
    outs = list(pipe.stream(iter(xs), on_forward=lambda k, x: model(x)))
    assert len(outs) == 3
    for got, w_k in zip(outs, want):
        for g_, w_ in zip(got, w_k):
            _same_people(g_, w_)
    torch.cuda.synchronize()
