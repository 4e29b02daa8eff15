"""``AttentionStudent(body_half=True)`` on an MI355X (run with -m gpu).

Per op, exact: the fp16 forms of avgpool, se, cam_combine and sigmoid_add (csrc/student_ops.hip), and the fp16 convs the
teacher never ran - dilations 2 to 5 into 32-channel slices of an in-place concat, the 1x1 over that concat, the biased 3x3
heads - each on a small fp16 program with the ``any_size`` property, against the float64 references of
tests/test_student_half_host.py (whose rounding points are PyTorch-CPU's, asserted there) by ``array_equal``.  The data is
order-independent (see that file).  x, both outputs and the workspace sit between guard bands, the outputs preset to a NaN
pattern and the workspace to a finite sentinel: a store outside a tensor and an element an op never writes both show.

The two sigmoids have no single right bit pattern (``expf`` on the device is not correctly rounded): they are compared
with the float64 sigmoid rounded to fp16, and the neighbouring fp16 value is admitted only where the float64 value lies
within the fp32 sigmoid budget (4 + |argument| fp32 ulps, oracle/student_ops.py) of the rounding boundary; such elements are
at most 1 % of a case (about 0.1 % by ulp counting, asserted on the CPU).

Whole network: the fixture of the reference's CPU half path (tests/golden/student_half.npz) with the criteria of DESIGN.md
section 2; StudentPipeline on a half model; and the default model's bits, recorded before the keyword existed."""
import os

import numpy as np
import pytest
import torch

import test_student_half_host as H
import test_student_ops_host as T
from oracle import exact, synth
from test_conv_exact_gpu import _same
from test_student_ops_gpu import Net
from test_student_pipeline_gpu import _expanded, _parser
from test_student_pipeline_gpu import _same as _same_people
from test_student_sizes_gpu import _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = torch.float64
J = 17
MAP_IDS = lambda s: "n%d_%dx%d" % s if isinstance(s, tuple) and len(s) == 3 else str(s)


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


def _f32(t):
    """fp16 values read through a selection head with fp32 NCHW output (which reads -0 as +0)"""
    return (t + 0.0).float().contiguous().numpy()


def _fed(fd):
    """an fp16 program up to the op's input: stem, then the feed's 3x3 stride-2 layer (the map at 1/4)"""
    net = Net(f32=False)
    t = net.b.stem(fd.stem.stem[0], fd.stem.stem[1])
    t = net.b.conv(t, fd.layer[0], fd.layer[1], relu=False)
    assert net.b.tensors[t] == [fd.x.shape[1], 2, 2]
    return net, t


def _layer_op(net, t, layer, relu=False):
    return net.b.conv(t, layer[0], layer[1], relu=relu)


def _sigmoid16_ok(got, arg, what):
    ok, near, took = H.sigmoid16_check(torch.from_numpy(np.ascontiguousarray(got)).double(), arg)
    print("%s: %.3f %% of the elements lie within the budget of a rounding boundary, %d took the neighbouring value"
          % (what, 100 * near, took))
    assert ok and near <= 0.01, what


# --------------------------------------------------------------------------- #
# avgpool
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", H.OP_MAPS, ids=MAP_IDS)
@pytest.mark.parametrize("C", H.OP_CHANNELS)
def test_avgpool_fp16_is_exact(nat, C, shape):
    """rows of 8 and of 104 channels (100 used: the pad channels are pooled zeros) on 9 x 12, 12 x 9 and 16 x 24 maps"""
    N, Hh, W = shape
    fd = H.feed(N, Hh, W, C, min(C, 100), "unit")
    net, t = _fed(fd)
    y = net.b.avgpool(t)
    assert net.b.tensors[y] == [C, 3, 2]
    net.head(y, range(C), 0)
    ref = H.avgpool16(fd.x, fd.quantum)
    got = _run(nat, net, N, Hh, W, x=fd.stem.x.half())
    _same(got[0], _f32(ref.out), "avgpool fp16 C=%d %s (divisors %s)" % (C, shape, ref.counts))
    if C > 100:
        assert not got[0][:, 100:].any()


# --------------------------------------------------------------------------- #
# se + cam_combine
# --------------------------------------------------------------------------- #
def _fc(w, b):
    fc = torch.nn.Linear(w.shape[1], w.shape[0])
    with torch.no_grad():
        fc.weight.copy_(w.float()); fc.bias.copy_(b.float())
    return fc.half()


def _const_layer(ld, value):
    return T.make_layer(torch.zeros(ld, ld, 1, 1, dtype=D), torch.ones(ld, dtype=D), torch.full((ld,), value, dtype=D), 1)


@pytest.mark.parametrize("shape", H.OP_MAPS, ids=MAP_IDS)
@pytest.mark.parametrize("case", H.se_cases(), ids=lambda c: "C%d_hid%d_ld%d" % c)
def test_se_gate_and_cam_combine_fp16(nat, case, shape):
    """the gate row, read through cam_combine(ones, zeros, gate): one row per image, zeros beyond channel C, every gate the
    float64 sigmoid of the reference logit rounded to fp16 (or its neighbour next to a rounding boundary); and
    cam_combine(hdc, res, gate) of the EMITTED gates, exact.  H * W is 108 or 384: no multiple of 64 on the ragged maps"""
    C, hid, ld = case
    N, Hh, W = shape
    d = H.se_data(C, hid, ld, shape)
    net, x = _fed(d.feed)
    gate = net.b.se(x, _fc(d.w1, d.b1), _fc(d.w2, d.b2))
    assert net.b.tensors[gate] == [ld, -1, 2]
    ones, zeros = _layer_op(net, x, _const_layer(ld, 1.0)), _layer_op(net, x, _const_layer(ld, 0.0))
    net.head(net.b.cam_combine(ones, zeros, gate), range(ld), 0)
    res, hdc = _layer_op(net, x, d.l_res), _layer_op(net, x, d.l_hdc)
    net.head(net.b.cam_combine(hdc, res, gate), range(ld), 1)
    got = _run(nat, net, N, Hh, W, x=d.feed.stem.x.half())
    what = "se fp16 C=%d hid=%d ld=%d %s" % (C, hid, ld, shape)
    rows = got[0][:, :, 0, 0]
    _same(got[0], np.ascontiguousarray(np.broadcast_to(rows[:, :, None, None], got[0].shape)), what + ": one gate per image")
    _same(rows[:, C:], np.zeros((N, ld - C), np.float32), what + ": padding channels of the gate row")
    _sigmoid16_ok(rows[:, :C], d.ref.logit, what)
    emitted = torch.from_numpy(np.ascontiguousarray(rows)).double()
    assert H.is_f16(emitted)
    _same(got[1], _f32(H.cam16(d.res, d.hdc, emitted)), what + ": combine of the emitted gates")


# --------------------------------------------------------------------------- #
# sigmoid_add
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", H.OP_MAPS, ids=MAP_IDS)
@pytest.mark.parametrize("C", H.OP_CHANNELS)
def test_sigmoid_add_fp16(nat, C, shape):
    N, Hh, W = shape
    d = H.sig_data(C, shape)
    net, x = _fed(d.feed)
    lg = _layer_op(net, x, d.l_logit)
    y = net.b.sigmoid_add(lg, x, out_flag=net.nat.F_OUT_PREDS)
    net.shapes[0] = (1, 2)
    net.head(y, range(C), 1)
    got = _run(nat, net, N, Hh, W, x=d.feed.stem.x.half())
    what = "sigmoid_add fp16 C=%d %s" % (C, shape)
    _sigmoid16_ok(got[0], H.sigadd_arg(d.logits), what)
    att = torch.from_numpy(got[0]).double()
    _same(got[1], _f32(H.sigadd16(d.x, att)), what + ": x + the emitted map")


# --------------------------------------------------------------------------- #
# fp16 convs the teacher never ran
# --------------------------------------------------------------------------- #
CONV_MAPS = [(2, 33, 47), (1, 80, 80)]                # maps 9 x 12 (a dilation-5 halo is wider than the map) and 20 x 20


def _dilated(layer, d):
    layer[0].dilation, layer[0].padding = (d, d), (d, d)
    return layer


@pytest.mark.parametrize("shape", CONV_MAPS, ids=MAP_IDS)
def test_dilated_fp16_convs_into_slices_and_the_1x1_over_them_are_exact(nat, shape):
    """conv 3x3 104 -> 25 + BN + ReLU at dilations 1 to 5, each stored as 32 channels into slice d - 1 of a 160-wide tensor
    (channels 25..31 of a slice: zeros), then conv 1x1 160 -> 100 + BN + ReLU over the concat with re-indexed weights, as
    ContextAwareModule.emit lays them out; every conv on the one-workgroup-per-tile kernel"""
    N, Hh, W = shape
    fd = H.feed(N, Hh, W, 104, 100, "mixed")
    g = H._g(5, N, Hh, W)
    net, x = _fed(fd)
    cat = net.b.new_tensor(160, 2)
    want = torch.zeros((N, 160) + tuple(fd.x.shape[2:]), dtype=D)
    for d in range(1, 6):
        w = torch.zeros(25, 104, 3, 3, dtype=D)
        w[:, :100] = H._ints(g, -1, 1, (25, 100, 3, 3))
        alpha = torch.tensor([0.0625, 0.125])[torch.randint(0, 2, (25,), generator=g)].double()
        layer = _dilated(T.make_layer(w, alpha, H._ints(g, -16, 16, (25,)) / 8, 1), d)
        net.b.conv(x, layer[0], layer[1], relu=True, out=(cat, 32 * (d - 1)), cout_store=32)
        assert 900 * float(fd.x.abs().max()) / fd.quantum < 2 ** 24
        want[:, 32 * (d - 1):32 * (d - 1) + 25] = exact.reference(fd.x, layer[2], layer[3], layer[4], None, 3, 1, d, True, True).out
    net.head(cat, range(160), 0)
    wt = torch.zeros(100, 160, 1, 1, dtype=D)
    cols = torch.tensor([c for c in range(160) if c % 32 < 25])
    wt[:, cols] = H._ints(g, -1, 1, (100, 125, 1, 1))
    top = T.make_layer(wt, torch.full((100,), 0.25, dtype=D), H._ints(g, -16, 16, (100,)) / 8, 1)
    q = 2.0 ** -7                                          # (multiples of 1/8 times alpha >= 1/16, rounded to fp16: coarser or equal)
    assert torch.equal(torch.round(want / q) * q, want) and (want > 0).double().mean() > 0.2
    y = net.b.conv(cat, top[0], top[1], relu=True)
    assert net.b.tensors[y] == [104, 2, 2]
    net.head(y, range(104), 1)
    want_top = T.ref_layer(want, top, 1, 1, True, q)
    got = _run(nat, net, N, Hh, W, x=fd.stem.x.half())
    for d in range(1, 6):
        s = slice(32 * (d - 1), 32 * d)
        _same(got[0][:, s], _f32(want[:, s]), "conv 3x3 104 -> 25 dilation %d into slice %d, %s" % (d, d - 1, shape))
    _same(got[1][:, :100], _f32(want_top), "conv 1x1 160 -> 100 over the concat, %s" % (shape,))
    assert not got[1][:, 100:].any()


@pytest.mark.parametrize("shape", CONV_MAPS, ids=MAP_IDS)
def test_biased_fp16_heads_are_exact(nat, shape):
    """conv 3x3 104 -> 1 and 104 -> 18 with a bias and no BatchNorm, fp32 NCHW outputs: one rounding behind the bias"""
    N, Hh, W = shape
    d1, d18 = H.head_data(1, shape), H.head_data(18, shape)
    net, x = _fed(d1.feed)
    for k, d in enumerate((d1, d18)):
        conv = torch.nn.Conv2d(104, d.w.shape[0], 3, 1, 1)
        with torch.no_grad():
            conv.weight.copy_(d.w.float()); conv.bias.copy_(d.bias.float())
        net.b.conv(x, conv.half(), None, out_flag=(nat.F_OUT_PREDS, nat.F_OUT_REFINED)[k], nhwc=False)
        net.shapes[k] = (d.w.shape[0], 2)
    got = _run(nat, net, N, Hh, W, x=d1.feed.stem.x.half())
    _same(got[0], _f32(d1.want), "head 104 -> 1, %s" % (shape,))
    _same(got[1], _f32(d18.want), "head 104 -> 18, %s" % (shape,))


# --------------------------------------------------------------------------- #
# a second trip of every grid-stride loop
# --------------------------------------------------------------------------- #
def test_every_fp16_grid_stride_loop_takes_a_second_trip(nat):
    """N = 9 at 512 x 512 on the stem's 64-channel map (256 x 256): cam_combine and sigmoid_add get 4.7 M pieces of 16 bytes,
    avgpool 1.18 M, against the 4,096 x 256 that one trip covers.  The SE gates are 0, 0.5 and 1 (zero second layer, biases
    -110, 0, 20), the sigmoid's arguments stay within +-1.9, so the pooled sums are exact."""
    N, Hh, W, C = 9, 512, 512, 64
    assert N * 128 * 128 * (C // 8) > T.ONE_TRIP
    f = T.stem_feed(N, Hh, W)
    g = H._g(6)
    net = Net(f32=False)
    t = net.b.stem(f.stem[0], f.stem[1])
    w1, b1 = H._ints(g, -1, 1, (16, C)), H._ints(g, -3, 3, (16,))
    b2 = torch.tensor([0.0, 20.0, -110.0], dtype=D)[torch.arange(C) % 3]
    gate = net.b.se(t, _fc(w1, b1), _fc(torch.zeros(C, 16, dtype=D), b2))
    cam = net.b.cam_combine(t, t, gate)
    l_logit = T.make_layer(H.sparse_weights(g, 8, C, 1, 2), torch.full((8,), 0.25, dtype=D), H._ints(g, -8, 8, (8,)) / 8, 1)
    lg = net.b.conv(t, l_logit[0], l_logit[1], relu=False)
    y = net.b.sigmoid_add(lg, cam, out_flag=nat.F_OUT_PREDS)
    net.shapes[0] = (1, 1)
    net.head(net.b.avgpool(y), range(C), 1)
    gates = torch.tensor([0.5, 1.0, 0.0], dtype=D)[torch.arange(C) % 3].view(1, C).expand(N, C).contiguous()
    r_cam = H.cam16(f.out, f.out, gates)
    logits = H.apply1x1(f.out, l_logit)[:, :1]
    arg = H.sigadd_arg(logits)
    assert float(arg.abs().max()) <= 1.9
    got = _run(nat, net, N, Hh, W, x=f.x.half())
    _sigmoid16_ok(got[0], arg, "large program: the sigmoid map")
    r_y = H.sigadd16(r_cam, torch.from_numpy(got[0]).double())
    _same(got[1], _f32(H.avgpool16(r_y, 2.0 ** -13).out), "large program: avgpool of the summed map")


# --------------------------------------------------------------------------- #
# refusals before the first launch
# --------------------------------------------------------------------------- #
def test_fp16_ops_refuse_rows_that_are_no_multiple_of_eight(nat):
    """an fp16 avgpool into a 12-channel tensor: RTPE_E_INVALID and untouched outputs"""
    fd = H.feed(1, 33, 47, 8, 8, "unit")
    net, x = _fed(fd)
    y = net.b.new_tensor(12, 3)
    net.b._op("avgpool3s2 C=8", kind=nat.OP_AVGPOOL, in_t=x, out_t=y, cin=8, cout=8)
    net.head(x, range(8), 0)
    rc = _run(nat, net, 1, 33, 47, x=fd.stem.x.half(), expect_error=True)
    msg = nat.lib().rtpe_last_error_string().decode()
    assert rc != 0 and "multiple of 8" in msg, (rc, msg)


# --------------------------------------------------------------------------- #
# whole student
# --------------------------------------------------------------------------- #
_STUDENTS = {}


def _half_student(golden_dir, weights):
    """the seeded W1 student with a half body; "bundled": the bundled attention weights on top (tests/golden/
    student_half_bundled_*.npz: mid_stem and att_*, as tools/gen_golden_student_half.py loaded them)"""
    if weights not in _STUDENTS:
        from rtpe.students import AttentionStudent
        import test_student_sizes_host as S
        stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False, body_half=True).eval()
        stu.load_state_dict(S.student_sd(golden_dir, "s100"), strict=True)
        if weights == "bundled":
            sd = {}
            for part in "abc":
                z = np.load(os.path.join(golden_dir, "student_half_bundled_%s.npz" % part))
                sd.update({k: torch.from_numpy(z[k]) for k in z.files})
            res = stu.load_state_dict(sd, strict=False)
            assert not res.unexpected_keys and all(k.split(".")[0] in ("stem", "det_lo", "det_mid", "det_hi", "det_top") or
                                                   k.endswith("num_batches_tracked") for k in res.missing_keys)
            assert "mid_stem.0.weight" in sd and "att_lo.1.se.fc.0.bias" in sd
        _STUDENTS[weights] = stu.to(DEV)
    return _STUDENTS[weights]


def _criteria(got, g, name, key):
    """DESIGN.md section 2 for one map: (1) max |HIP - half reference| <= 1.25 x the reference's self-spread max + one fp16 step of
    the map's range; (2) mean <= 1.15 x its self-spread mean where that is nonzero; (3) against the fp32 reference: max <= 1.25 x
    max |CPU-half - fp32| + one fp16 step, mean <= 1.15 x mean |CPU-half - fp32|"""
    half, f32 = g["%s_%s_half" % (name, key)].astype(np.float32), g["%s_%s_f32" % (name, key)]
    sp_max, sp_mean = g["%s_%s_spread" % (name, key)]
    assert got.shape == half.shape and got.dtype == np.float32
    assert np.array_equal(got.astype(np.float16).astype(np.float32), got), "%s %s: a value is no fp16 number" % (name, key)
    rng = float(np.abs(half).max())
    step = 2.0 ** (np.floor(np.log2(rng)) - 10)
    err, own = np.abs(got - half), np.abs(half - f32)
    e32 = np.abs(got - f32)
    print("%s %s: range %.3f, one fp16 step %.2e | HIP vs half reference max %.3e mean %.3e | reference vs itself max %.3e mean "
          "%.3e | HIP vs fp32 reference max %.3e mean %.3e | half reference vs fp32 reference max %.3e mean %.3e"
          % (name, key, rng, step, err.max(), err.mean(), sp_max, sp_mean, e32.max(), e32.mean(), own.max(), own.mean()))
    assert err.max() <= 1.25 * sp_max + step, (name, key, "criterion 1")
    if sp_mean > 0:
        assert err.mean() <= 1.15 * sp_mean, (name, key, "criterion 2")
    assert e32.max() <= 1.25 * own.max() + step and e32.mean() <= 1.15 * own.mean(), (name, key, "criterion 3")


@pytest.mark.parametrize("case", H.HALF_CASES, ids=lambda c: c[0])
def test_half_student_vs_the_reference_half_fixture(nat, golden_dir, case):
    """the reference's CPU half path per case and per map.  64 x 96 runs the tuned routes, 33 x 47 and 100 x 140 the general
    kernels.  Figures of the first run on an MI355X: see the printed lines (pytest -s)."""
    name, weights, n, h, w, seed = case
    g = np.load(os.path.join(golden_dir, "student_half.npz"))
    stu = _half_student(golden_dir, weights)
    x = synth.make_images(n, h, w, seed=seed).to(DEV)
    with torch.no_grad():
        att, det = stu(x)
    assert att.dtype == torch.float32 and det.dtype == torch.float32
    _criteria(att.cpu().numpy(), g, name, "att")
    _criteria(det.cpu().numpy(), g, name, "det")


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_student_pipeline_on_a_half_student(nat, golden_dir, match_on):
    """StudentPipeline takes the half model unchanged: per image bit-identical to parse_lowres on the model's own expanded
    det; stream() equals __call__"""
    from rtpe.engine import StudentPipeline
    stu = _half_student(golden_dir, "W1")
    xs = [synth.make_images(2, 96, 128, seed=60 + k).to(DEV) for k in range(3)]
    want = []
    for x in xs:
        with torch.no_grad():
            att, det = stu(x)
        assert det.shape == (2, J + 1, 24, 32) and det.dtype == torch.float32
        want.append(_parser(match_on).parse_lowres(*_expanded(det.float()), (96, 128)))
    pipe = StudentPipeline(stu, _parser(match_on), DEV)
    call = [pipe(x) for x in xs]
    streamed = list(pipe.stream(iter(xs), in_flight=2))
    assert len(streamed) == 3
    for k in range(3):
        assert len(call[k]) == 2 == len(streamed[k]) == len(want[k])
        for c, s, w_ in zip(call[k], streamed[k], want[k]):
            _same_people(c, w_)
            _same_people(s, w_)


def test_the_default_student_gives_the_bits_it_gave_before(nat, golden_dir):
    """body_half=False on the 33 x 47 case of student_sizes.npz: tests/golden/student_default_33x47.npz holds the outputs of
    the commit before the keyword existed, recorded on an MI355X"""
    from rtpe.students import AttentionStudent
    import test_student_sizes_host as S
    g = np.load(os.path.join(golden_dir, "student_default_33x47.npz"))
    for kw in ({}, {"body_half": False}):
        stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False, **kw).eval()
        stu.load_state_dict(S.student_sd(golden_dir, "s100"), strict=True)
        with torch.no_grad():
            att, det = stu.to(DEV)(synth.make_images(2, 33, 47, seed=101).to(DEV))
        _same(att.cpu().numpy(), g["att"], "default student, att")
        _same(det.cpu().numpy(), g["det"], "default student, det")
