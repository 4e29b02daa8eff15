"""The students' eight small fp32 ops, each on a small program of its own (run with -m gpu on an MI355X).

``RTPE_OP_CAST``, ``AVGPOOL``, ``SE``, ``CAM_COMBINE``, ``SIGMOID_ADD``, ``AUX_PACK``, ``RESIZE`` and ``GATE_MUL``
(csrc/student_ops.hip, dispatched in csrc/engine.hip) against the float64 references of oracle/student_ops.py.  The data
comes from tests/test_student_ops_host.py: integers far below 2^24 carried to the op by the fp16 stem (the cast and
avgpool cases) or by the second input and 1x1 / centre-tap stride-2 fp32 convs with weights in {-1, 0, 1}, and read
back through fp32 1x1 heads with 0/1 selection weights (NCHW outputs) - convs that are exact in any order on this data.

Which comparison is which:

  cast          exact (fp16 denormals, +-65504, negatives, zeros).
  avgpool       exact: the exact window sum divided by the number of taps inside, one rounding.
  aux_pack      exact: a copy plus a zero channel.  (A selection head turns -0 into +0, so the sign of a zero is not seen.)
  resize        exact: PyTorch-CPU's half-pixel bilinear with every fp32 operation rounded once; the neighbouring channels of
                the target tensor, which a conv writes before the op in one case and after it in the other, stay exact.
  se            the gate, read through cam_combine with res = 0 and hdc = 1: exact where the integer logit is 0 (0.5),
                >= 18 (1.0) or <= -104 (0.0), and inside the sigmoid budget on the generic logits; the padding channels of
                the gate row are zero.
  cam_combine   exact given the gate row the kernel emitted: relu(fp32(res + fp32(hdc * gate))) on integer res and hdc, and
                exact end to end on the channels whose gate is 0, 0.5 or 1.
  sigmoid_add,  the emitted NCHW map: exact at the exact points, inside the budget elsewhere.  The NHWC result equals
  gate_mul      fp32(x + att) / fp32(x * att) of the EMITTED map bit for bit - a consistency check that never stands alone.

The sigmoid budget is ``4 + |argument|`` ulps of the fp32 result for |argument| <= 80, derived, not measured: the division
``l / div`` leaves the argument with a relative error of 2^-24, which e^-a turns into up to |a| ulps; 1 ulp is the bound
of ``expf`` in the HIP math API reference (table of the single precision functions), half an ulp each for the add and the
divide, one for ulp boundaries.  Arguments in (-104, -80) are kept out of the data (denormal results).

Every forward runs with x, the second input, both outputs and the workspace between guard bands; the outputs are preset to
a NaN pattern and the workspace to a finite sentinel, so a store outside a tensor and an element an op never writes both
show.  The kernels of the feeding convs are the defaults.  Shapes are the smallest at which a kernel can go wrong, plus one
large program (N = 5, 512 x 512) in which every grid-stride loop takes a second trip."""
import ctypes
import types

import numpy as np
import pytest
import torch

import test_student_ops_host as T
from oracle import exact
from oracle import student_ops as so
from test_conv_exact_gpu import _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_SENTINEL = 12345.0            # finite as fp32 and as two fp16 halves (6.25, -1024): a selection head stays exact over it
D = torch.float64


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


# --------------------------------------------------------------------------- #
# programs
# --------------------------------------------------------------------------- #
class Net:
    """a ProgramBuilder with fp32 convs made from explicit integer weights"""

    def __init__(self, f32):
        from rtpe.third_party.pose_higher_hrnet import ProgramBuilder
        from rtpe import _native
        self.b = ProgramBuilder(f32=f32)
        self.nat = _native
        self.shapes = [None, None]               # channels and ds of the two NCHW outputs

    @staticmethod
    def _conv(w, bias, stride):
        import torch.nn as nn
        cout, cin, k, _ = w.shape
        conv = nn.Conv2d(cin, cout, k, stride, k // 2, bias=bias is not None)
        with torch.no_grad():
            conv.weight.copy_(w.float())
            if bias is not None:
                conv.bias.copy_(bias.float())
        return conv

    def conv(self, t, w, bias=None, stride=1, into=None, coff=0):
        """fp32 conv of tensor t (all its physical channels); ``into``: channels [coff, coff + cout) of that tensor"""
        assert self.b.f32 and w.shape[1] == self.b.tensors[t][0], (w.shape, self.b.tensors[t])
        if into is None:
            return self.b.conv(t, self._conv(w, bias, stride), None)
        assert w.shape[0] % 4 == 0 and coff + w.shape[0] <= self.b.tensors[into][0]
        return self.b.conv(t, self._conv(w, bias, stride), None, out=(into, coff), cout_store=w.shape[0])

    def tensor(self, t, width, w, bias=None):
        """a new tensor of exactly ``width`` channels at t's resolution, filled by a 1x1 conv of t"""
        assert w.shape[0] == width
        out = self.b.new_tensor(width, self.b.tensors[t][1])
        self.conv(t, w, bias, into=out)
        return out

    def chain(self, ds):
        """the packed second input and its ``ds`` sub-sampled copies (test_student_ops_host.aux_feed)"""
        ts = [self.b.aux_input()]
        for _ in range(ds):
            ts.append(self.conv(ts[-1], T.sub_weights(self.b.tensors[ts[-1]][0]), None, 2))
        return ts

    def head(self, t, chans, which):
        """NCHW output ``which`` (0: preds, 1: refined) = the physical channels ``chans`` of tensor t"""
        chans = list(chans)
        w = torch.zeros(len(chans), self.b.tensors[t][0], 1, 1, dtype=D)
        for i, c in enumerate(chans):
            w[i, c] = 1
        flag = (self.nat.F_OUT_PREDS, self.nat.F_OUT_REFINED)[which]
        self.b.conv(t, self._conv(w, None, 1), None, out_flag=flag, nhwc=False)
        self.shapes[which] = (len(chans), self.b.tensors[t][1])

    def linear(self, w, bias):
        import torch.nn as nn
        fc = nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            fc.weight.copy_(w.float()); fc.bias.copy_(bias.float())
        return fc


def _ws_guarded(nbytes):
    """the workspace between two guard bands, all of it preset to the finite sentinel"""
    ge = 65536 // 4
    n = (nbytes + 255) // 256 * 256 // 4
    bits = int(torch.tensor([WS_SENTINEL]).view(torch.int32)[0])
    buf = torch.full((2 * ge + n,), bits, dtype=torch.int32, device=DEV)
    view = buf[ge:ge + n]
    assert view.data_ptr() % 256 == 0
    return types.SimpleNamespace(buf=buf, t=view, lo=ge, hi=ge + n, bits=bits)


def _run(nat, net, N, H, W, x=None, aux=None, expect_error=False):
    """one forward of the finished program on guarded x, aux, outputs and workspace; returns the two outputs (numpy) - or
    the return code with ``expect_error`` - after checking every guard band"""
    from rtpe.third_party.pose_higher_hrnet import Engine
    prog = net.b.finish()
    eng = Engine(prog, 0)
    L = nat.lib()
    if x is None:
        x = torch.zeros(N, 3, H, W, dtype=torch.float16)
    xg = exact.guarded(x.contiguous(), exact.IN_SENTINEL)
    ag = exact.guarded(aux.float().contiguous(), exact.IN_SENTINEL) if aux is not None else None
    assert bool(getattr(prog, "has_aux", False)) == (aux is not None)
    outs = []
    for s_ in net.shapes:
        shape = (N, s_[0], H >> s_[1], W >> s_[1]) if s_ else (1, 1, 1, 64)
        outs.append(exact.guarded_out(shape, torch.float32))
    need = ctypes.c_size_t()
    nat.check(L.rtpe_hrnet_workspace_bytes(eng._h, N, H, W, ctypes.byref(need)))
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
        return rc
    nat.check(rc)
    got = [o.t.cpu().numpy() for o in outs]
    for o, s_ in zip(got, net.shapes):
        if s_ is None:                           # an output the program does not have stays untouched
            assert (o.view(np.int32) == np.int32(exact.OUT_PATTERN[4])).all()
    return got


def _f32np(t):
    """the expected fp32 array of values read through a selection head (which reads -0 as +0: the sum starts at +0)"""
    return (t + 0.0).float().contiguous().numpy()


def _sigmoid_ok(got, logits, div, what):
    """the emitted sigmoid values against the integer logits: exact points and budget; prints the largest error"""
    ok, ulps, at, share, wrong = so.sigmoid_check(torch.from_numpy(np.ascontiguousarray(got)).double(), logits, div)
    print("%s: largest error %.2f ulps at argument %.2f; %.0f %% of the budget of 4 + |a| ulps; %d wrong exact points"
          % (what, ulps, at, 100 * share, wrong))
    assert ok, what


# --------------------------------------------------------------------------- #
# cast
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", T.CAST_CASES, ids=lambda c: "n%d_%dx%d" % c)
def test_cast_is_exact(nat, case):
    """fp16 -> fp32 behind the stem and a 1x1 fp16 conv without ReLU, as the students emit it (ld == C in every product
    program: test_student_ops_host asserts that)"""
    N, H, W = case
    d = T.cast_data(N, H, W)
    net = Net(f32=False)
    t = net.b.stem(d.feed.stem[0], d.feed.stem[1])
    t = net.b.conv(t, d.layer[0], d.layer[1], relu=False)
    t = net.b.cast(t)
    net.b.f32 = True
    net.head(t, range(0, 32), 0)
    net.head(t, range(32, 64), 1)
    got = _run(nat, net, N, H, W, x=d.feed.x.half())
    _same(got[0], _f32np(d.want[:, :32]), "cast %s channels 0..31" % (case,))
    _same(got[1], _f32np(d.want[:, 32:]), "cast %s channels 32..63" % (case,))


# --------------------------------------------------------------------------- #
# avgpool
# --------------------------------------------------------------------------- #
AVGPOOL_PARAMS = [(C, m) for C, _ in T.emitted().avgpool for m in T.AVGPOOL_MAPS]


@pytest.mark.parametrize("C,m", AVGPOOL_PARAMS, ids=lambda v: "C%d" % v if isinstance(v, int) else "n%d_%dx%d_ds%d_%s" % v)
def test_avgpool_is_exact(nat, C, m):
    """every (C, ld) the four product programs emit (C == ld) x maps 16 x 16, 48 x 16 and 2 x 2 (divisors 4, 6, 9)"""
    N, H, W, ds, feed = m
    d = T.avgpool_data(C, N, H, W, ds, feed)
    if feed == "stem":
        net = Net(f32=False)
        t = net.b.cast(net.b.stem(d.feed.stem[0], d.feed.stem[1]))
        net.b.f32 = True
        x, aux = d.feed.x.half(), None
    else:
        net = Net(f32=True)
        t = net.chain(ds)[-1]
        x, aux = None, d.aux
    t = net.b.avgpool(net.tensor(t, C, d.w, d.bias))
    assert tuple(net.b.tensors[t][:2]) == (C, ds + 1)
    half = C // 2
    net.head(t, range(0, half), 0)
    net.head(t, range(half, C), 1)
    got = _run(nat, net, N, H, W, x=x, aux=aux)
    what = "avgpool C=%d %s (divisors %s)" % (C, m, d.ref.counts)
    _same(got[0], _f32np(d.ref.out[:, :half]), what)
    _same(got[1], _f32np(d.ref.out[:, half:]), what)


@pytest.mark.parametrize("m", T.AVGPOOL_REFUSED, ids=lambda m: "n%d_%dx%d_ds%d" % m)
def test_avgpool_of_a_map_with_an_odd_side_is_an_error_return(nat, m):
    """a 2 x 1 or 1 x 1 map pools into 1 x 1, but the output tensor of the program holds (H >> ds + 1) x (W >> ds + 1) = no
    pixel at all: the forward returns an error instead of writing beyond the tensor"""
    N, H, W, ds = m
    net = Net(f32=True)
    ch = net.chain(ds)
    net.b.avgpool(ch[-1])
    net.head(ch[0], range(4), 0)
    rc = _run(nat, net, N, H, W, aux=torch.zeros(N, 3, H, W), expect_error=True)
    msg = nat.lib().rtpe_last_error_string().decode()
    assert rc != 0 and "avgpool: a %d x %d map does not pool" % (H >> ds, W >> ds) in msg, (rc, msg)


# --------------------------------------------------------------------------- #
# se + cam_combine
# --------------------------------------------------------------------------- #
def _se_program(C, hid, in_ld, zero_cols, ds, wx, bx, w1, b1, w2, b2, w_res, b_res, w_hdc, b_hdc):
    net = Net(f32=True)
    src = net.chain(ds)[-1]
    x = net.tensor(src, in_ld, wx, bx)
    if zero_cols:                                # the re-indexed form of ContextAwareModule.emit(col_map=...)
        gate = net.b.se(x, net.linear(torch.zeros(hid, C - len(zero_cols), dtype=D), b1), net.linear(w2, b2), w1=w1.float())
    else:
        gate = net.b.se(x, net.linear(w1, b1), net.linear(w2, b2))
    gl = net.b.tensors[gate][0]
    zero_w = torch.zeros(gl, 8, 1, 1, dtype=D)
    ones = net.tensor(src, gl, zero_w, torch.ones(gl, dtype=D))
    zeros = net.tensor(src, gl, zero_w, torch.zeros(gl, dtype=D))
    net.head(net.b.cam_combine(ones, zeros, gate), range(gl), 0)
    res, hdc = net.tensor(src, gl, w_res, b_res), net.tensor(src, gl, w_hdc, b_hdc)
    net.head(net.b.cam_combine(hdc, res, gate), range(gl), 1)
    return net, gl


@pytest.mark.parametrize("case", T.se_cases(), ids=lambda c: "C%d_hid%d_ld%d_z%d_hw%d" % (c[0], c[1], c[2], len(c[3]), c[4]))
def test_se_gate_and_cam_combine(nat, case):
    """every (C, hid, row width) the product programs emit, the re-indexed w1 included, C = 264 and the limits (512, 128);
    HW in {1, 2, 3, 6, 256}; three images with different means"""
    C, hid, in_ld, zero_cols, HW = case
    d = T.se_data(*case)
    net, gl = _se_program(C, hid, in_ld, zero_cols, d.ds, d.wx, d.bx, d.w1, d.b1, d.w2, d.b2, d.w_res, d.b_res, d.w_hdc, d.b_hdc)
    assert gl == d.gl
    got = _run(nat, net, d.N, d.H, d.W, aux=d.aux)
    what = "se C=%d hid=%d ld=%d hw=%d" % (C, hid, in_ld, HW)
    rows = got[0][:, :, 0, 0]                                       # the gate row of every image
    _same(got[0], np.ascontiguousarray(np.broadcast_to(rows[:, :, None, None], got[0].shape)), what + ": one gate per image")
    _same(rows[:, C:], np.zeros((d.N, gl - C), np.float32), what + ": padding channels of the gate row")
    _sigmoid_ok(rows[:, :C], d.ref.logit, None, what)
    emitted = torch.from_numpy(np.ascontiguousarray(rows)).double()
    _same(got[1], _f32np(so.cam_combine(d.res, d.hdc, emitted)), what + ": combine of the emitted gates")
    # end to end where the gate has one right value
    ex = so.sigmoid_map(d.ref.logit).exact
    want = so.cam_combine(d.res[:, :C], d.hdc[:, :C], d.ref.gate.float().double())
    sel = ex[:, :, None, None].expand_as(want).numpy()
    assert np.array_equal(got[1][:, :C][sel].view(np.int32), _f32np(want)[sel].view(np.int32)), what + ": exact gates"


@pytest.mark.parametrize("case", T.SE_REFUSED, ids=lambda c: "C%d_hid%d" % c[:2])
def test_se_beyond_its_limits_is_an_error_return(nat, case):
    C, hid, in_ld = case
    g = torch.Generator().manual_seed(T.SEED + C + hid)
    r = lambda *shape: torch.randint(-1, 2, shape, generator=g).double()
    gl = (C + 7) // 8 * 8
    wz = torch.zeros(gl, 8, 1, 1, dtype=D)
    net, _ = _se_program(C, hid, in_ld, (), 5, torch.zeros(in_ld, 8, 1, 1, dtype=D), r(in_ld), r(hid, C), r(hid), r(C, hid), r(C),
                         wz, r(gl), wz, r(gl))
    rc = _run(nat, net, 1, 32, 32, aux=torch.zeros(1, 3, 32, 32), expect_error=True)
    msg = nat.lib().rtpe_last_error_string().decode()
    assert rc != 0 and ("se: C=%d hidden=%d unsupported" % (C, hid)) in msg, (rc, msg)


# --------------------------------------------------------------------------- #
# sigmoid_add, gate_mul
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("C,_", T.SIGMOID_ADD_CASES, ids=str)
def test_sigmoid_add(nat, C, _):
    d = T.sig_data(C, 20.0)
    net = Net(f32=True)
    a = net.b.aux_input()
    lg = net.conv(a, d.w_l)
    x = net.tensor(a, C, d.w_x, d.b_x)
    y = net.b.sigmoid_add(lg, x, out_flag=net.nat.F_OUT_PREDS)
    net.shapes[0] = (1, 0)
    net.head(y, range(C), 1)
    got = _run(nat, net, d.N, d.H, d.W, aux=d.aux)
    _sigmoid_ok(got[0], d.logits, 20.0, "sigmoid_add C=%d" % C)
    att = torch.from_numpy(got[0]).double()
    _same(got[1], _f32np(so.sigmoid_add(d.x, att)), "sigmoid_add C=%d: x + the emitted map" % C)


@pytest.mark.parametrize("P,div,order", T.GATE_MUL_CASES, ids=str)
def test_gate_mul_into_a_channel_range(nat, P, div, order):
    """gate_mul into channels [0, P + 4) of a (2P + 4)-wide tensor whose channels [P + 4, 2P + 4) a conv writes before the op
    in one case and after it in the other"""
    d = T.sig_data(P + 4, div, 1)
    w_n, b_n = T.gate_mul_neighbour(P)
    net = Net(f32=True)
    a = net.b.aux_input()
    lg = net.conv(a, d.w_l)
    x = net.tensor(a, P + 4, d.w_x, d.b_x)
    cat2 = net.b.new_tensor(2 * P + 4, 0)
    if order == "before":
        net.conv(a, w_n, b_n, into=cat2, coff=P + 4)
    net.b.gate_mul(lg, x, cat2, P + 4, div, out_flag=net.nat.F_OUT_PREDS)
    net.shapes[0] = (1, 0)
    if order == "after":
        net.conv(a, w_n, b_n, into=cat2, coff=P + 4)
    net.head(cat2, range(2 * P + 4), 1)
    got = _run(nat, net, d.N, d.H, d.W, aux=d.aux)
    what = "gate_mul P=%d div=%s neighbour written %s" % (P, div, order)
    _sigmoid_ok(got[0], d.logits, div, what)
    att = torch.from_numpy(got[0]).double()
    want = torch.cat([so.gate_mul(d.x, att), so.exact_conv(d.packed, w_n, b_n)], 1)
    _same(got[1], _f32np(want), what + ": x * the emitted map | the neighbour's channels")


# --------------------------------------------------------------------------- #
# aux_pack, resize
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", T.AUX_PACK_CASES, ids=lambda c: "n%d_%dx%d" % c)
def test_aux_pack_is_exact(nat, case):
    N, H, W = case
    d = T.aux_pack_data(N, H, W)
    net = Net(f32=True)
    net.head(net.b.aux_input(), range(4), 0)
    got = _run(nat, net, N, H, W, aux=d.aux)
    _same(got[0], _f32np(d.want), "aux_pack %s" % (case,))


@pytest.mark.parametrize("case", T.RESIZE_CASES, ids=lambda c: "ds%d_to_ds%d_n%d_%dx%d_%s" % c)
def test_resize_into_a_channel_range(nat, case):
    """ratios 4, 2, 8, 1 and the upscales 1/2 and 1/4 on 32 x 96 inputs, into channels [P, P + 4) beside a conv's"""
    s, t, N, H, W, order = case
    d = T.resize_data(s, t, N, H, W)
    clamp0, edge, shortcut = T.resize_expect(s, t)
    for ax in (d.ref.y, d.ref.x):
        assert (ax.clamp0, ax.edge, ax.shortcut) == (clamp0, edge, shortcut)
    P = T.RESIZE_P
    net = Net(f32=True)
    ch = net.chain(d.top)
    tgt = net.b.new_tensor(P + 4, t)
    if order == "before":
        net.conv(ch[t], d.w_n, d.b_n, into=tgt)
    net.b.resize(ch[s], tgt, P, 4)
    if order == "after":
        net.conv(ch[t], d.w_n, d.b_n, into=tgt)
    net.head(tgt, range(P + 4), 0)
    got = _run(nat, net, N, H, W, aux=d.aux)
    _same(got[0], _f32np(d.want), "resize %s" % (case,))


# --------------------------------------------------------------------------- #
# more than one trip of every grid-stride loop
# --------------------------------------------------------------------------- #
def test_every_grid_stride_loop_takes_a_second_trip(nat):
    """one program with all eight ops at N = 5, 512 x 512: every grid-stride kernel gets more work items than the 4,096 x 256
    one launch covers in one trip.  The logits sit at the exact points only and the SE gates are 0, 0.5 and 1, so the whole
    chain cast -> cam_combine -> sigmoid_add -> gate_mul -> avgpool, with aux_pack and resize feeding the combine's
    residual, has one right answer."""
    N, H, W = T.LARGE
    C = 64
    for op, items in T.large_items(N, H, W, C).items():
        assert items > T.ONE_TRIP, (op, items)
    g = torch.Generator().manual_seed(T.SEED + 99)
    ints = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    f = T.stem_feed(N, H, W)
    # the second input: plane 0 holds logits that are exact with and without the division by 20
    pts = torch.tensor([0.0, 360.0, 400.0, 5000.0, -2080.0, -2100.0, -9000.0], dtype=D)
    aux = torch.cat([pts[torch.randint(0, len(pts), (N, 1, H, W), generator=g)], ints(-4, 4, N, 2, H, W)], 1)
    packed = so.aux_pack(aux)
    w_t, b_t = ints(-1, 1, 8, 4, 1, 1), ints(-3, 3, 8)
    w_t[:, 0] = 0                                                           # (the logits stay out of the data path)
    w_d, b_d = ints(-1, 1, C, 12, 3, 3), ints(-3, 3, C)
    w_d[:, 8] = 0
    w_lg = torch.zeros(1, 4, 3, 3, dtype=D)
    w_lg[0, 0, 1, 1] = 1
    w_c, b_c = ints(-1, 1, C, 64, 1, 1), ints(-3, 3, C)
    hid = 16
    w1, b1, w2 = ints(-1, 1, hid, C), ints(-3, 3, hid), torch.zeros(C, hid, dtype=D)
    b2 = torch.tensor([0.0, 20.0, -110.0], dtype=D)[torch.arange(C) % 3]

    net = Net(f32=False)
    F_ = net.b.cast(net.b.stem(f.stem[0], f.stem[1]))
    net.b.f32 = True
    a = net.b.aux_input()
    t0 = net.b.new_tensor(12, 0)
    net.conv(a, w_t, b_t, into=t0)
    net.b.resize(a, t0, 8, 4)
    dn = net.conv(t0, w_d, b_d, stride=2)
    lg = net.conv(a, w_lg, None, stride=2)
    c1 = net.conv(F_, w_c, b_c)
    gate = net.b.se(c1, net.linear(w1, b1), net.linear(w2, b2))
    cam = net.b.cam_combine(c1, dn, gate)
    sa = net.b.sigmoid_add(lg, cam)
    y = net.b.new_tensor(C, 1)
    net.b.gate_mul(lg, sa, y, C, None, out_flag=net.nat.F_OUT_PREDS)
    net.shapes[0] = (1, 1)
    net.head(net.b.avgpool(y), range(C), 1)

    r_t0 = torch.cat([so.exact_conv(packed, w_t, b_t), so.resize(packed, H, W).out], 1)
    r_dn = so.exact_conv(r_t0, w_d, b_d, 2)
    logits = so.exact_conv(packed, w_lg, None, 2)[:, :1]
    r_c1 = so.exact_conv(so.cast(f.out), w_c, b_c, 1, False, f.quantum)
    gates = so.sigmoid_map(b2).want.view(1, C).expand(N, C).contiguous()
    r_cam = so.cam_combine(r_dn, r_c1, gates)
    s20, s1 = so.sigmoid_map(logits, 20.0), so.sigmoid_map(logits, None)
    assert s20.exact.all() and s1.exact.all() and torch.equal(s20.want, s1.want)
    r_y = so.gate_mul(so.sigmoid_add(r_cam, s20.want), s1.want)
    assert (r_y != 0).double().mean() > 0.3
    want = so.avgpool(r_y).out
    got = _run(nat, net, N, H, W, x=f.x.half(), aux=aux)
    _same(got[0], _f32np(s1.want), "large program: the sigmoid map")
    _same(got[1], _f32np(want), "large program: avgpool of the gated map")
