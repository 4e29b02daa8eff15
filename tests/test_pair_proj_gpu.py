"""The skip projection of layer1's first Bottleneck computed inside the first 1x1 pair kernel (option "pair_proj",
csrc/conv_pair.hip PROJ; RTPE_F_PAIR_PROJ): exact against the float64 reference of oracle/exact.py, as a program and as a
single launch, folded and not, and the whole network with the fold on against off (GPU tests: run with -m gpu on an
MI355X; the program compiler's part needs none).

Pixel counts.  A forward takes inputs whose sides are multiples of 32 (rtpe_hrnet_forward refuses anything else), so a
map of a program holds a multiple of 256 pixels at /2 and of 64 at /4: through a program the pair kernel never sees a
partial 16-pixel tile, and never fewer tiles than a workgroup has waves except at the smallest input.  The partial-tile
cases (15 pixels: one partial tile; 105 pixels: seven tiles for eight waves, the last one partial) therefore run through
the layer-level entry rtpe_conv1x1_pair_nhwc on the same layers and the same reference; the program runs at 3 x 64 x 96
and at 2 x 256 x 320 (40,960 pixels at /2 > 256 workgroups x 8 waves x 16 pixels: every wave of the first workgroups
loops, so the one-tile-ahead prefetch of x is used behind the first tile) and, in the network test, at 1 x 32 x 32 (64
pixels at /4: four tiles for eight waves)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import exact, synth
from test_conv_exact_gpu import DEV, SEED, _Options, _affine_is_exact, _forward, _layer, _nhwc, _ref_layer, _same

FPT = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


class _Opts(_Options):
    DEFAULTS = dict(_Options.DEFAULTS, pair_proj=1)


def _layers(g, side=False):
    stem, skip = _layer(3, 64, 3, 2, g), _layer(64, 256, 1, 1, g)
    head, tail = _layer(64, 256, 1, 1, g), _layer(256, 64, 1, 1, g)
    outs = [_layer(64, 34, 1, 1, g, bn=False), _layer(64, 17, 1, 1, g, bn=False)]
    extra = [_layer(256, 64, 1, 1, g)] if side else []
    assert all(_affine_is_exact(l) for l in [stem, skip, head, tail] + outs + extra)
    return stem, skip, head, tail, outs, extra


def _program(nat, layers):
    """stem -> projection -> [second reader of the projection's output] -> head with residual = projection -> tail -> the two
    output heads (the second one on the second reader's output when there is one); returns (engine, index of the projection)"""
    from rtpe.third_party.pose_higher_hrnet import Engine, ProgramBuilder
    stem, skip, head, tail, outs, extra = layers
    b = ProgramBuilder(f32=False)
    t64 = b.stem(stem[0], stem[1])
    t256 = b.conv(t64, skip[0], skip[1], relu=False)
    ts = b.conv(t256, extra[0][0], extra[0][1], relu=True) if extra else None
    th = b.conv(t64, head[0], head[1], relu=True, residual=t256)
    tt = b.conv(th, tail[0], tail[1], relu=True)
    b.conv(tt, outs[0][0], None, out_flag=nat.F_OUT_PREDS, nhwc=False)
    b.conv(ts if extra else tt, outs[1][0], None, out_flag=nat.F_OUT_REFINED, nhwc=False)
    prog = b.finish()
    ih = 3 if extra else 2
    assert prog.ops[ih].flags & nat.F_PAIR_HEAD and prog.ops[ih + 1].flags & nat.F_PAIR_TAIL
    assert bool(prog.ops[1].flags & nat.F_PAIR_PROJ) == (not extra)
    return Engine(prog, 0), 1


def _reference(x, layers):
    stem, skip, head, tail, outs, extra = layers
    y64 = _ref_layer(x.double(), stem, 3, 2, True, True, quantum=1.0)
    y256 = _ref_layer(y64, skip, 1, 1, False, True, quantum=0.5)
    yh = _ref_layer(y64, head, 1, 1, True, True, res=y256, quantum=0.5)
    yt = _ref_layer(yh, tail, 1, 1, True, True, quantum=0.25)
    ys = _ref_layer(y256, extra[0], 1, 1, True, True, quantum=0.25) if extra else None
    want = [_ref_layer(yt, outs[0], 1, 1, False, False, quantum=0.125).float().numpy(),
            _ref_layer(ys if extra else yt, outs[1], 1, 1, False, False, quantum=0.125).float().numpy()]
    return want


def _run_program(nat, shape, side):
    N, H, W = shape
    g = torch.Generator().manual_seed(SEED + 3 * H + W + (7 if side else 0))
    layers = _layers(g, side)
    eng, ip = _program(nat, layers)
    x = torch.randint(-3, 4, (N, 3, H, W), generator=g).half()
    want = _reference(x, layers)                         # once per shape, shared by the four settings
    xg = exact.guarded(x, exact.IN_SENTINEL)
    shapes = [(N, 34, H // 2, W // 2), (N, 17, H // 2, W // 2)]
    for proj in (0, 1):
        for pair in (0, 1):
            with _Opts(nat, pair_proj=proj, pair_1x1=pair):
                folded = eng.op_tile(ip, N, H, W)[0] == 0
                pg, rg = _forward(nat, eng, xg, N, H, W, shapes)
            what = "1x1 pair program n%d %dx%d side=%d pair_proj=%d pair_1x1=%d" % (N, H, W, side, proj, pair)
            # folded exactly when both options are on and nobody else reads the projection's output
            assert folded == bool(proj and pair and not side), what
            _same(pg.t.cpu().numpy(), want[0], what + " head 34")
            _same(rg.t.cpu().numpy(), want[1], what + " head 17")
            assert exact.guards_intact(xg, pg, rg), what


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 64, 96), (2, 256, 320)], ids=lambda s: "n%d_%dx%d" % s)
def test_folded_projection_program_is_exact(nat, shape):
    """the program of test_1x1_pair_is_exact under pair_proj x pair_1x1; rtpe_hrnet_op_tile reports the projection without a
    launch of its own exactly when both are on"""
    _run_program(nat, shape, side=False)


@pytest.mark.gpu
def test_projection_with_a_second_reader_is_not_folded(nat):
    """a conv 256 -> 64 reads the projection's output too (its result feeds the second output head): the program compiler
    does not flag the projection, it runs as a launch of its own under every setting, and the outputs are exact"""
    _run_program(nat, (3, 64, 96), side=True)


def _conv(nat, x, layer, relu, res, y):
    conv, norm, w, alpha, beta = layer
    al, be = alpha.float().contiguous(), beta.float().contiguous()
    wh = conv.weight.detach().half().contiguous()
    nat.check(nat.lib().rtpe_conv2d_nhwc(x.data_ptr(), x.shape[0], x.shape[1], x.shape[2], x.shape[3], wh.data_ptr(),
                                         ctypes.cast(al.data_ptr(), FPT), ctypes.cast(be.data_ptr(), FPT), wh.shape[0], 1, 1,
                                         nat.F_ROUND_CONV | (nat.F_RELU if relu else 0), res.data_ptr() if res is not None else None,
                                         y.data_ptr(), nat.stream_ptr(torch.device(DEV))))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 5), (3, 5, 7)], ids=lambda s: "n%d_%dx%d" % s)
def test_folded_projection_launch_is_exact_on_partial_tiles(nat, shape):
    """15 pixels (one partial tile) and 105 pixels (seven tiles for eight waves, the last one partial) - pixel counts no program
    has - through rtpe_conv1x1_pair_nhwc: projection folded, projection as a launch of its own into the pair's residual, and
    three launches, all against the float64 reference; guards around every tensor"""
    N, H, W = shape
    g = torch.Generator().manual_seed(SEED + 31 * H + W)
    skip, head, tail = _layer(64, 256, 1, 1, g), _layer(64, 256, 1, 1, g), _layer(256, 64, 1, 1, g)
    # x as the stem's output is (multiples of 1/2, the first Bottleneck's input), t another such tensor (conv2's output)
    x = (torch.randint(-40, 41, (N, 64, H, W), generator=g).float() / 2).half()
    t = (torch.randint(0, 41, (N, 64, H, W), generator=g).float() / 2).half()
    d = _ref_layer(x.double(), skip, 1, 1, False, True, quantum=0.5)
    yw = _ref_layer(t.double(), head, 1, 1, True, True, res=d, quantum=0.5)
    uw = _ref_layer(yw, tail, 1, 1, True, True, quantum=0.25)
    yw, uw = _nhwc(yw).half().numpy(), _nhwc(uw).half().numpy()
    L = nat.lib()
    packs = []
    for conv, norm, w, alpha, beta in (head, tail, skip):
        packs.append((conv.weight.detach().half().contiguous(), alpha.float().contiguous(), beta.float().contiguous()))
    for proj, pair in ((1, 1), (0, 1), (0, 0)):
        xg, tg = exact.guarded(_nhwc(x), exact.IN_SENTINEL), exact.guarded(_nhwc(t), exact.IN_SENTINEL)
        dg, yg, ug = [exact.guarded_out((N, H, W, c), torch.float16) for c in (256, 256, 64)]
        if not proj:
            _conv(nat, xg.t, skip, False, None, dg.t)
        if pair:
            args = [tg.t.data_ptr(), None if proj else dg.t.data_ptr(), xg.t.data_ptr() if proj else None, N, H, W]
            for k, (wh, al, be) in enumerate(packs):
                args += [wh.data_ptr(), al.data_ptr(), be.data_ptr()] if (k < 2 or proj) else [None, None, None]
            nat.check(L.rtpe_conv1x1_pair_nhwc(*args, yg.t.data_ptr(), ug.t.data_ptr(), nat.stream_ptr(torch.device(DEV))))
        else:
            _conv(nat, tg.t, head, True, dg.t, yg.t)
            _conv(nat, yg.t, tail, True, None, ug.t)
        torch.cuda.synchronize()
        what = "1x1 pair launch n%d %dx%d pair_proj=%d pair_1x1=%d" % (N, H, W, proj, pair)
        _same(yg.t.cpu().numpy(), yw, what + " y")
        _same(ug.t.cpu().numpy(), uw, what + " u")
        assert exact.guards_intact(xg, tg, yg, ug) and (proj or exact.guards_intact(dg)), what


@pytest.mark.gpu
def test_folded_projection_does_not_change_the_network_output(nat, w48_shapes):
    """whole network, half wrapper: pair_proj 0 against 1, bit for bit, at the sizes of
    test_1x1_pairs_do_not_change_the_network_output and at the smallest input (1 x 32 x 32: 64 pixels at /4, four tiles for
    the eight waves of one workgroup); repeated: the projection's input shares no slot with what the pair writes"""
    from rtpe.helpers import build_hrnet_w48_teacher
    L = nat.lib()
    sd = synth.make_state_dict(w48_shapes, 0, "W1")
    m = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(DEV)
    try:
        for n, hw in ((1, (64, 96)), (3, (160, 224)), (2, (96, 32)), (5, (128, 128)), (1, (32, 32))):
            x = synth.make_images(n, hw[0], hw[1], seed=70 + n).to(DEV)
            nat.check(L.rtpe_set_option(b"pair_proj", 0))
            with torch.no_grad():
                p0, r0 = m(x)
            eng = m[1]._engine(torch.device(DEV))
            ip = [i for i, o in enumerate(eng.program.ops) if o.flags & nat.F_PAIR_PROJ]
            assert len(ip) == 1 and eng.op_tile(ip[0], n, hw[0], hw[1])[0] != 0
            nat.check(L.rtpe_set_option(b"pair_proj", 1))
            assert eng.op_tile(ip[0], n, hw[0], hw[1])[0] == 0
            for rep in range(2):
                with torch.no_grad():
                    p1, r1 = m(x)
                assert torch.equal(p0, p1) and torch.equal(r0, r1), (n, hw, rep)
    finally:
        nat.check(L.rtpe_set_option(b"pair_proj", 1))


def test_program_promises_the_projection_input_over_the_first_pair():
    """the compiled w48 teacher carries RTPE_F_PAIR_PROJ on exactly one op, the producer of the first pair head's residual, and
    no tensor that is first touched before the end of that pair's tail shares the workspace slot of that op's input"""
    from rtpe import _native as nat
    from rtpe.helpers import build_hrnet_w48_teacher
    prog = build_hrnet_w48_teacher()[1].compile_program()
    ops = list(prog.ops)
    flagged = [i for i, o in enumerate(ops) if o.flags & nat.F_PAIR_PROJ]
    assert len(flagged) == 1
    p = flagged[0]
    heads = [i for i, o in enumerate(ops) if o.flags & nat.F_PAIR_HEAD]
    assert len(heads) == 3 and ops[heads[0]].res_t == ops[p].out_t and p < heads[0]
    tail = heads[0] + 1
    assert ops[tail].flags & nat.F_PAIR_TAIL
    assert (ops[p].cin, ops[p].cout, ops[p].ksize, ops[p].stride) == (64, 256, 1, 1)
    x_t = ops[p].in_t

    def touched(o):
        return [t for t in [o.out_t, o.res_t, o.in_t if o.kind != nat.OP_FUSE else -1] + [o.term_t[k] for k in range(o.n_terms)]
                if t >= 0]
    first = {}
    for i, o in enumerate(ops):
        for t in touched(o):
            first.setdefault(t, i)
    slot = prog.tensors[x_t].slot
    assert first[x_t] <= p
    for t, i in first.items():
        if t != x_t and prog.tensors[t].slot == slot:
            assert i < first[x_t] or i > tail, "tensor %d (first touched at op %d) shares the slot of the projection's input" % (t, i)
