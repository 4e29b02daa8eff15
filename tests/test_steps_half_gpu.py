"""``AttentionStudentStepsHalf`` on an MI355X (run with -m gpu).

Per op, exact: the fp16 forms of aux_pack, resize and gate_mul (csrc/student_ops.hip) and the two 5x5 stride-2 fp16 convs of the
alt stem, each on a small fp16 program with the ``any_size`` property, against the float64 references of
tests/test_steps_half_host.py (whose rounding points are PyTorch-CPU's, asserted there) by ``array_equal``.  x, the second
input, both outputs and the workspace sit between guard bands, the outputs preset to a NaN pattern and the workspace to a
finite sentinel: a store outside a tensor and an element an op never writes both show.  Read-back goes through fp16 selection
heads, as in tests/test_student_half_gpu.py.

The emitted sigmoid map has no single right bit pattern (``expf`` on the device is not correctly rounded): the kernel rounds
an fp32 value that lies within the fp32 sigmoid budget (4 + |argument| fp32 ulps, oracle/student_ops.py) of the true sigmoid
once to fp16, so it must give the correctly rounded half of the true value unless the true value lies within that budget of
the boundary between two halves, where either neighbour is admitted (``sigmoid16_check``); such elements are at most 1 % of
a case (0.1 to 0.4 % by ulp counting, asserted on the CPU).  Where the logit gives 0.5, 1 or 0 no boundary is near: exact.

Whole network: the fixture of the reference's CPU half path (tests/golden/steps_half.npz) with the criteria of DESIGN.md
section 2; StudentPipeline and eval_student on the half model; the schedule checker on one traced forward."""
import os

import numpy as np
import pytest
import torch

import test_steps_half_host as S
import test_student_half_host as H
import test_student_ops_host as T
from oracle import synth
from test_conv_exact_gpu import _same
from test_student_half_gpu import _criteria, _f32, _sigmoid16_ok
from test_student_ops_gpu import Net
from test_student_pipeline_gpu import _expanded, _n_people, _parser
from test_student_pipeline_gpu import _same as _same_people
from test_student_sizes_gpu import _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = torch.float64
J = 17
E_INVALID = -1                                          # RTPE_E_INVALID (include/rtpe_hip.h)


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


def _op(net, t, layer, relu=False, **kw):
    return net.b.conv(t, layer[0], layer[1], relu=relu, **kw)


def _chain(net, ds):
    """the packed fp16 second input and its ``ds`` sub-sampled copies (rows of 8)"""
    ts = [net.b.aux_input(half=True)]
    for _ in range(ds):
        ts.append(_op(net, ts[-1], S.sub_layer()))
    return ts


# --------------------------------------------------------------------------- #
# aux_pack
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", S.PACK_CASES, ids=lambda c: "n%d_%dx%d" % c)
def test_aux_pack_fp16_is_exact(nat, case):
    """ties to even, values of 16 significant bits, a value that becomes an fp16 denormal; five zero pad channels"""
    N, Hh, W = case
    d = S.pack_data(N, Hh, W, True)
    net = Net(f32=False)
    a = net.b.aux_input(half=True)
    assert net.b.tensors[a] == [8, 0, 2]
    net.head(a, range(8), 0)
    got = _run(nat, net, N, Hh, W, aux=d.aux)
    _same(got[0], _f32(d.want), "aux_pack fp16 %s" % (case,))
    assert not got[0][:, 3:].any()


# --------------------------------------------------------------------------- #
# resize
# --------------------------------------------------------------------------- #
def _resize_program(net, ch, s, t, l_n, order):
    P = S.RESIZE_P
    tgt = net.b.new_tensor(P + 8, t)
    if order == "before":
        _op(net, ch[t], l_n, out=(tgt, 0), cout_store=P)
    net.b.resize(ch[s], tgt, P, 8, half=True)
    if order == "after":
        _op(net, ch[t], l_n, out=(tgt, 0), cout_store=P)
    net.head(tgt, range(P + 8), 0)


@pytest.mark.parametrize("case", S.RESIZE_CASES, ids=lambda c: "ds%d_to_ds%d_n%d_%dx%d_%s" % c)
def test_resize_fp16_into_a_channel_range(nat, case):
    """ratios 4, 2, 8, 1 and the upscales 1/2 and 1/4 on 32 x 96 inputs, into channels [P, P + 8) of a (P + 8)-wide tensor
    beside a conv's channels, written before the op in one case and after it in the other"""
    s, t, N, Hh, W, order = case
    d = S.resize_data(s, t, N, Hh, W)
    net = Net(f32=False)
    _resize_program(net, _chain(net, d.top), s, t, d.l_n, order)
    got = _run(nat, net, N, Hh, W, aux=d.aux)
    _same(got[0], _f32(d.want), "resize fp16 %s" % (case,))
    assert not got[0][:, S.RESIZE_P + 3:].any()                 # the five pad channels: interpolated zeros


@pytest.mark.parametrize("data", ["eighths", "lab"])
@pytest.mark.parametrize("order", ["before", "after"])
def test_resize_fp16_of_a_ragged_input(nat, order, data):
    """33 x 47 -> 9 x 12, the product's resize at a size that is no multiple of 32: scales that are no fp32 numbers, the
    clamp at the last row and column.  "lab": the fixture's own second input, on which the three fmas of the fp32 op give
    another half than PyTorch's order in one element (tests/test_steps_half_host.py)"""
    d = S.resize_ragged_data() if data == "eighths" else S.resize_lab_data()
    w = torch.zeros(S.RESIZE_P, 8, 1, 1, dtype=D)
    w[:, :2] = torch.eye(2, dtype=D).repeat(S.RESIZE_P // 2, 1).view(S.RESIZE_P, 2, 1, 1)          # copies: exact on any halves
    l_n = T.make_layer(w, torch.ones(S.RESIZE_P, dtype=D), torch.zeros(S.RESIZE_P, dtype=D), 1)
    net = Net(f32=False)
    _resize_program(net, _chain(net, 2), 0, 2, l_n, order)
    got = _run(nat, net, d.N, d.H, d.W, aux=d.aux)
    neigh = d.src[:, :2, ::4, ::4].repeat(1, S.RESIZE_P // 2, 1, 1)
    _same(got[0], _f32(torch.cat([neigh, d.out], 1)), "resize fp16 33 x 47 -> 9 x 12 (%s), neighbour written %s" % (data, order))


# --------------------------------------------------------------------------- #
# gate_mul
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("P,div,order", S.GATE_CASES, ids=str)
def test_gate_mul_fp16_into_a_channel_range(nat, P, div, order):
    """gate_mul into channels [0, P + 8) of a (2P + 8)-wide tensor whose channels [P + 8, 2P + 8) a conv writes before the op
    in one case and after it in the other; the product of the EMITTED map is exact"""
    d = S.gate_data(P, div)
    net = Net(f32=False)
    a = net.b.aux_input(half=True)
    lg, x = _op(net, a, d.l_logit), _op(net, a, d.l_x)
    assert net.b.tensors[x] == [P + 8, 0, 2]
    cat2 = net.b.new_tensor(2 * P + 8, 0)
    if order == "before":
        _op(net, a, d.l_n, out=(cat2, P + 8), cout_store=P)
    net.b.gate_mul(lg, x, cat2, P + 8, div, out_flag=nat.F_OUT_PREDS, half=True)
    net.shapes[0] = (1, 0)
    if order == "after":
        _op(net, a, d.l_n, out=(cat2, P + 8), cout_store=P)
    net.head(cat2, range(2 * P + 8), 1)
    got = _run(nat, net, d.N, d.H, d.W, aux=d.aux)
    what = "gate_mul fp16 P=%d div=%s neighbour written %s" % (P, div, order)
    _sigmoid16_ok(got[0], d.arg, what)
    arg = d.arg.numpy()
    for sel, v in ((arg == 0, 0.5), (arg >= 9, 1.0), (arg <= -18, 0.0)):           # no rounding boundary near: one right value
        assert sel.any() and (got[0][sel] == np.float32(v)).all(), (what, v)
    att = torch.from_numpy(got[0]).double()
    assert H.is_f16(att)
    _same(got[1], _f32(torch.cat([S.gate16(d.x, att), d.neigh], 1)), what + ": x * the emitted map | the neighbour's channels")


# --------------------------------------------------------------------------- #
# the two 5x5 stride-2 convs of the alt stem
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", S.CONV5_FIRST, ids=lambda s: "n%d_%dx%d" % s)
def test_the_5x5_stride_2_fp16_convs_are_exact(nat, shape):
    """conv 8 -> 56 (3 -> 50 logical) + BN + ReLU from the packed second input (output 0: 16 x 16 and 17 x 24), then conv
    56 -> 48 (50 logical) + BN + ReLU stored into channels [56, 104) of a 104-wide tensor whose channels [0, 56) another conv
    writes (output 1: 8 x 8 and 9 x 12).  32 x 32 takes the executor's routes, 33 x 47 the general kernel; both must run the
    one-workgroup-per-tile kernel (no fast family has 25 taps)"""
    from rtpe.third_party.pose_higher_hrnet import Engine
    N, Hh, W = shape
    d = S.conv5_data(N, Hh, W)
    net = Net(f32=False)
    a = net.b.aux_input(half=True)
    u = _op(net, a, d.l1, relu=True)
    assert net.b.tensors[u] == [56, 1, 2] and net.b.ops[-1].cin == 8
    net.head(u, range(56), 0)
    cat2 = net.b.new_tensor(104, 2)
    wk = torch.zeros(56, 56, 3, 3, dtype=D)
    wk[torch.arange(56), torch.arange(56), 1, 1] = 1
    keep = T.make_layer(wk, torch.ones(56, dtype=D), torch.zeros(56, dtype=D), 2)
    _op(net, u, keep, out=(cat2, 0), cout_store=56)
    _op(net, u, d.l2, relu=True, out=(cat2, 56), cout_store=48)
    assert net.b.ops[-1].cin == 56 and net.b.ops[-1].ksize == 5
    net.head(cat2, range(104), 1)
    # before the first launch: both layers on the tile kernel, within the LDS of a CU
    net.b.any_size = True
    eng = Engine(net.b.finish(), 0)
    k5 = [i for i, o in enumerate(eng.program.ops) if o.ksize == 5]
    assert len(k5) == 2
    for i in k5:
        lds = eng.op_tile(i, N, Hh, W)[7]
        assert 0 < lds <= 160 * 1024, (i, lds)
    del eng
    got = _run(nat, net, N, Hh, W, aux=d.aux)
    _same(got[0], _f32(d.u), "conv 5x5 s2 8 -> 56 %s" % (shape,))
    _same(got[1], _f32(torch.cat([d.u[:, :, ::2, ::2], d.v], 1)), "conv 5x5 s2 56 -> 48 into [56, 104) %s" % (shape,))


# --------------------------------------------------------------------------- #
# a second trip of every grid-stride loop
# --------------------------------------------------------------------------- #
def test_every_new_grid_stride_loop_takes_a_second_trip(nat):
    """N = 5 at 512 x 512, everything at full resolution: aux_pack gets 1.31 M pixels, the resize (ratio 1, 8 channels) 1.31 M
    pieces of 16 bytes, gate_mul (16 channels) 2.62 M, against the 4,096 x 256 that one trip covers.  The logits sit where the
    sigmoid is 0.5, 1 or 0, so the chain has one right answer; read back through an avgpool (a quarter of the bytes)."""
    N, Hh, W = T.LARGE
    assert N * Hh * W > T.ONE_TRIP
    g = S._g(7)
    pts = torch.tensor([0.0, 20.0, -30.0, 100.0, -104.0], dtype=D)
    aux = torch.cat([pts[torch.randint(0, len(pts), (N, 1, Hh, W), generator=g)], H._ints(g, -4, 4, (N, 2, Hh, W))], 1)
    packed = S.pack16(aux)
    w = torch.zeros(8, 8, 1, 1, dtype=D)
    w[:, 1:3] = H._ints(g, -1, 1, (8, 2, 1, 1))
    l_mix = T.make_layer(w, torch.ones(8, dtype=D), H._ints(g, -3, 3, (8,)), 1)
    w_l = torch.zeros(8, 8, 1, 1, dtype=D)
    w_l[0, 0] = 1
    l_logit = T.make_layer(w_l, torch.ones(8, dtype=D), torch.zeros(8, dtype=D), 1)
    net = Net(f32=False)
    a = net.b.aux_input(half=True)
    t0 = net.b.new_tensor(16, 0)
    _op(net, a, l_mix, out=(t0, 0), cout_store=8)
    net.b.resize(a, t0, 8, 8, half=True)
    lg = _op(net, a, l_logit)
    y = net.b.new_tensor(16, 0)
    net.b.gate_mul(lg, t0, y, 16, None, out_flag=nat.F_OUT_PREDS, half=True)
    net.shapes[0] = (1, 0)
    net.head(net.b.avgpool(y), range(16), 1)
    att = H.sigmoid16(aux[:, :1])
    assert set(att.unique().tolist()) == {0.0, 0.5, 1.0}
    r_y = S.gate16(torch.cat([H.apply1x1(packed, l_mix), packed], 1), att)
    assert (r_y != 0).double().mean() > 0.3
    got = _run(nat, net, N, Hh, W, aux=aux)
    _same(got[0], _f32(att), "large program: the sigmoid map")
    _same(got[1], _f32(H.avgpool16(r_y, 0.5).out), "large program: avgpool of the gated map")


# --------------------------------------------------------------------------- #
# refusals before the first launch
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("fault", ["offset", "row"])
def test_fp16_aux_ops_refuse_rows_and_offsets_that_are_no_multiple_of_eight(nat, fault):
    """a resize into channels [4, 12) of a 16-wide tensor; a gate_mul into a 12-wide tensor: RTPE_E_INVALID, outputs untouched"""
    net = Net(f32=False)
    a = net.b.aux_input(half=True)
    if fault == "offset":
        t = net.b.new_tensor(16, 0)
        net.b.resize(a, t, 4, 8, half=True)
        want = "offsets must be multiples of 8"
    else:
        t = net.b.new_tensor(12, 0)
        net.b.gate_mul(a, a, t, 8, None, out_flag=nat.F_OUT_PREDS, half=True)
        net.shapes[0] = (1, 0)
        want = "multiple of 8"
    net.head(a, range(8), 1)
    rc = _run(nat, net, 1, 32, 32, aux=torch.zeros(1, 3, 32, 32), expect_error=True)
    msg = nat.lib().rtpe_last_error_string().decode()
    assert rc == E_INVALID and want in msg, (rc, msg)


def test_an_fp16_packed_input_of_fewer_than_eight_channels_is_refused_at_create(nat):
    from rtpe.third_party.pose_higher_hrnet import Engine
    net = Net(f32=False)
    t = net.b.new_tensor(4, 0, 2)
    net.b._op("aux input 3->4", kind=nat.OP_AUX_PACK, in_t=-1, out_t=t, cin=3, cout=4)
    net.b.has_aux = True
    with pytest.raises(RuntimeError, match="packed second input"):
        Engine(net.b.finish(), 0)


# --------------------------------------------------------------------------- #
# whole student
# --------------------------------------------------------------------------- #
_STUDENTS = {}


steps_alt = S.steps_alt


def _fresh(P, wseed):
    from rtpe.students import AttentionStudentStepsHalf
    stu = AttentionStudentStepsHalf(None, "cpu", P, 17, 1, True, None, False).eval()
    stu.load_state_dict(S.steps_sd(P, wseed), strict=True)
    return stu.to(DEV)


def _half_steps(P, wseed):
    if (P, wseed) not in _STUDENTS:
        _STUDENTS[(P, wseed)] = _fresh(P, wseed)
    return _STUDENTS[(P, wseed)]


@pytest.mark.parametrize("case", S.STEPS_HALF_CASES, ids=lambda c: c[0])
def test_half_steps_student_vs_the_reference_half_fixture(nat, golden_dir, case):
    """the reference's CPU half path per case and per map, the three criteria of DESIGN.md section 2.  64 x 96 and 64 x 64 run
    the tuned routes, 33 x 47 the general kernels.  Also: the k = 5 convs sit on the tile kernel within the LDS of a CU (asked
    before the first forward), a second forward gives the same bits, and image 0 alone gives the bits it has in the batch.
    Figures on an MI355X (HIP vs half reference | reference vs itself; max, mean; the printed lines of pytest -s hold the rest):
      p48_33x47_nodiv  att 4.88e-4, 2.26e-6 | 4.88e-4, 2.26e-6   det 9.77e-4, 8.89e-5 | 9.77e-4, 9.56e-5
      p48_33x47_div20  att 0, 0 | 0, 0                             det 4.88e-4, 6.46e-5 | 4.88e-4, 6.72e-5
      p48_64x96_nodiv  att 4.88e-4, 3.82e-6 | 4.88e-4, 3.50e-6   det 9.77e-4, 9.74e-5 | 9.77e-4, 9.24e-5
      p48_64x96_div20  att 4.88e-4, 1.27e-6 | 4.88e-4, 1.27e-6   det 4.88e-4, 8.33e-5 | 5.49e-4, 7.95e-5
      p80_64x64_div20  att 4.88e-4, 1.91e-6 | 4.88e-4, 3.82e-6   det 4.88e-4, 7.01e-5 | 4.88e-4, 7.86e-5
    (With the fp32 op's three fmas in the fp16 resize, p48_33x47_nodiv missed criterion 2 on ``att``: 1.243e-5 against
    1.15 x 2.26e-6, from ONE element of the resized LAB image one fp16 step off; see tests/test_steps_half_host.py.)"""
    name, P, wseed, n, h, w, seed, alt_seed, div = case
    g = np.load(os.path.join(golden_dir, "steps_half.npz"))
    stu = _half_steps(P, wseed)
    eng = stu._engine(torch.device(DEV), ("att_divisor", div))
    k5 = [i for i, o in enumerate(eng.program.ops) if o.ksize == 5]
    assert len(k5) == 2 and all(0 < eng.op_tile(i, n, h, w)[7] <= 160 * 1024 for i in k5), [eng.op_tile(i, n, h, w) for i in k5]
    x, alt = synth.make_images(n, h, w, seed=seed).to(DEV), steps_alt(n, h, w, alt_seed).to(DEV)
    kw = {} if div is None else {"att_divisor": div}
    with torch.no_grad():
        att, det = [t.clone() for t in stu(x, alt=alt, **kw)]
        again = stu(x, alt=alt, **kw)
        first = stu(x[:1], alt=alt[:1], **kw)
    assert att.dtype == torch.float32 and det.dtype == torch.float32
    _criteria(att.cpu().numpy(), g, name, "att")
    _criteria(det.cpu().numpy(), g, name, "det")
    assert torch.equal(again[0], att) and torch.equal(again[1], det), "a second forward differs"
    assert torch.equal(first[0], att[:1]) and torch.equal(first[1], det[:1]), "image 0 alone differs from image 0 in the batch"


def test_a_forward_after_a_ragged_one_equals_a_fresh_modules(nat):
    """64 x 96 after 33 x 47 on one module against 64 x 96 on a new one: no state of the ragged forward (workspace, routes,
    launch shapes) reaches the next"""
    name, P, wseed, n, h, w, seed, alt_seed, div = S.STEPS_HALF_CASES[2]
    x, alt = synth.make_images(n, h, w, seed=seed).to(DEV), steps_alt(n, h, w, alt_seed).to(DEV)
    xr, ar = synth.make_images(2, 33, 47, seed=121).to(DEV), steps_alt(2, 33, 47, 122).to(DEV)
    used, fresh = _half_steps(P, wseed), _fresh(P, wseed)
    with torch.no_grad():
        used(xr, alt=ar)
        a1, d1 = used(x, alt=alt)
        a2, d2 = fresh(x, alt=alt)
    assert torch.equal(a1, a2) and torch.equal(d1, d2)
    with pytest.raises(NotImplementedError, match="ATM alt is expected"):
        used(x)


def test_the_c_entry_refuses_a_mixed_batch_of_a_half_aux_program(nat):
    """rtpe_hrnet_forward_mixed_aux on the half program: RTPE_E_INVALID before the first launch (outputs and workspace
    untouched), the message names the missing masked forms; the Python entries refuse before that"""
    from rtpe.students import pack_mixed
    from test_steps_mixed_gpu import _forward_mixed_aux_raw
    stu = _half_steps(48, 4)
    eng = stu._engine(torch.device(DEV), ("att_divisor", None))
    sizes = [(33, 47), (64, 40)]
    canvas, _ = pack_mixed([torch.rand(3, hh, ww) for hh, ww in sizes])
    rc = _forward_mixed_aux_raw(nat, eng, [(1, 2), (18, 2)], canvas, canvas * 50, sizes, expect_error=True)
    msg = nat.lib().rtpe_last_error_string().decode()
    assert rc == E_INVALID and "no masked form" in msg, (rc, msg)
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        stu.forward_mixed(canvas.to(DEV), sizes, alt=canvas.to(DEV))


# --------------------------------------------------------------------------- #
# pipeline, eval, schedule
# --------------------------------------------------------------------------- #
def test_student_pipeline_streams_the_half_steps_student(nat):
    """four (x, alt) batches of 2 x 96 x 128, two forwards in flight: per image bit-identical to the batch forwarded on its
    own and decoded as eval_student decodes; people are found; the mixed entries refuse"""
    from rtpe.engine import StudentPipeline
    stu = _half_steps(48, 4)
    gen = torch.Generator().manual_seed(31)
    batches = [(synth.make_images(2, 96, 128, seed=40 + k).to(DEV),
                (torch.rand(2, 3, 96, 128, generator=gen) * 100.0).to(DEV)) for k in range(4)]
    want = []
    for x, alt in batches:
        with torch.no_grad():
            att, det = stu(x, alt=alt)
        assert det.shape == (2, J + 1, 24, 32) and det.dtype == torch.float32 and att.shape == (2, 1, 24, 32)
        want.append(_parser().parse_lowres(*_expanded(det.float()), (96, 128)))
    pipe = StudentPipeline(stu, _parser(), DEV)
    got = list(pipe.stream(iter(batches), in_flight=2))
    call = pipe(batches[1][0], alt=batches[1][1])
    assert len(got) == 4
    for k in range(4):
        assert len(got[k]) == 2 == len(want[k])
        for g_, w_ in zip(got[k], want[k]):
            _same_people(g_, w_)
    for g_, w_ in zip(call, want[1]):
        _same_people(g_, w_)
    assert sum(_n_people(r[0]) for k in range(4) for r in got[k]) >= 1, "every decode came back empty"
    ims = [b[0][0] for b in batches[:2]]
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        pipe.call_mixed(ims, alt=ims)
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        list(pipe.stream_mixed(iter([(ims, ims)])))


def test_eval_student_runs_the_half_steps_student(nat):
    """eval_student calls ``model(img, out_hw)``: the Steps students get their second input from a wrapper, as the
    reference's evaluation script computes it from the image"""
    from rtpe import engine
    stu = _half_steps(48, 4)

    class WithAlt:
        def eval(self):
            return self

        def __call__(self, img, out_hw=None):
            return stu(img, out_hw, alt=img * 100.0)

    class Data:
        def evaluate(self, preds, scores, *a):
            return {"images": len(preds)}, None

    class Loader(list):
        dataset = Data()

    loader = Loader((i, synth.make_images(1, 96, 128, seed=70 + i)) for i in range(2))
    assert engine.eval_student(WithAlt(), _parser(), loader, DEV) == {"images": 2}


def test_half_steps_forward_keeps_its_slot_lifetimes(nat, monkeypatch):
    """one traced forward at 64 x 64 and one at 33 x 47 pass the happens-before checker (oracle/schedule.py), default launch
    shapes, as tests/test_schedule_gpu.py asks of the other students"""
    from test_schedule_gpu import check_forward
    monkeypatch.setenv("RTPE_AUTOTUNE", "0")
    stu = _fresh(48, 4)
    eng = stu._engine(torch.device(DEV), ("att_divisor", 20.0))
    assert eng.program.has_aux
    for N, Hh, W in ((1, 64, 64), (1, 33, 47)):
        x = synth.make_images(N, Hh, W, seed=14).to(DEV)
        alt = (torch.rand(N, 3, Hh, W, generator=torch.Generator().manual_seed(15)) * 100).to(DEV)
        _, _, _, st = check_forward(eng, lambda: eng.forward(x.float(), torch.float32, aux=alt), "half steps %dx%d" % (Hh, W), lanes=False)
        print("half steps student %s: %s" % ((Hh, W), st))
