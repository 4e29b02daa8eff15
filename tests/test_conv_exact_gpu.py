"""Every conv kernel family against THE answer (run with -m gpu on an MI355X).

The inputs come from oracle/exact.py: data on which fp32 accumulation is exact in any order, so the float64 reference
with the half wrapper's rounding points is the one right bit pattern for any kernel - the one-workgroup-per-tile
kernel, every variant of it, and whatever replaces them.  Every comparison here is ``np.array_equal`` on the integer
view of ALL elements.  Every launch runs on tensors with guard bands (oracle.exact.guarded): input guards hold a large
finite value, so a read outside the tensor that reaches a sum shows up in the result; output guards and the output
itself are preset to a NaN pattern, so a store outside the tensor and an element never written show up too.  Guarded
are the tensors a caller hands over: x, res, y, and the input and the two outputs of a program.  What the library
allocates or lays out itself is not: the packed weights, and a program's workspace with the intermediates of the stem
and pair tests.

Shapes (output sizes; a stride-2 conv reads twice the size): below one tile (3x5, 5x7), one pixel over a tile on each
axis (9x17 and 17x33: the kernels' tiles are 8x8, 8x16, 16x8, 6x32, 8x32, 16x16, 16x32), ragged 23x37; N in {1, 3}; and
per persistent kernel one case in which every workgroup walks at least three units (`walked`)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import exact
import test_conv_exact_host as host
from test_conv_exact_host import CLASSES, F32_CLASSES, SEED, _layer, _ref_layer, regimes_of, seed_of
from test_gpu_parity import CONV_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FPT = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


def _same(got, want, what):
    """exact equality of all elements on the integer view; the first differences otherwise"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    it = np.int16 if got.itemsize == 2 else np.int32
    if not np.array_equal(got.view(it), want.view(it)):
        msg = "%s: %s" % (what, exact.first_differences(got, want))
        print(msg)
        raise AssertionError(msg)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class _Options:
    """option settings for one launch, restored to the defaults afterwards"""
    DEFAULTS = {"tile_dma": 1, "direct_1x1": 1, "conv64": 1, "conv48s2": 1, "block_pc": 1, "block_ring": 0, "deconv48": 1,
                "fused_stem": 1, "head_direct": 1, "pair_1x1": 1}

    def __init__(self, nat, **settings):
        self.nat, self.settings = nat, settings

    def __enter__(self):
        for k, v in self.settings.items():
            self.nat.check(self.nat.lib().rtpe_set_option(k.encode(), v))

    def __exit__(self, *a):
        for k in self.settings:
            self.nat.check(self.nat.lib().rtpe_set_option(k.encode(), self.DEFAULTS[k]))


def class_options(cls):
    """the settings of the options that apply to a layer class: tile_dma for all, and the class's own variant switch"""
    cin, cout, k, s = cls
    own = None
    if k == 1:
        own = "direct_1x1"
    elif cls == (64, 64, 3, 1):
        own = "conv64"
    elif cin == 48 and k == 3 and s == 2:
        own = "conv48s2"
    return [dict(tile_dma=d, **({own: v} if own else {})) for d in (0, 1) for v in ((0, 1) if own else (1,))]


def class_flags(cls):
    """(residual, relu) the class has in the network, from CONV_CASES"""
    rows = [c for c in CONV_CASES if c[:4] == cls]
    return any(c[6] for c in rows), any(c[7] for c in rows)


# --------------------------------------------------------------------------- #
# rtpe_conv2d_nhwc
# --------------------------------------------------------------------------- #
SHAPES = [(3, 5), (5, 7), (9, 17), (17, 33), (23, 37)]          # output H, output W


def shapes_of(i):
    """three (N, H, W) per class: one of the two shapes below a tile, one of the two a pixel over a tile, the ragged one.
    Shape and batch size alternate independently from class to class, and inside a class N goes 3, 1, 3 or 1, 3, 1: every
    class runs N = 1 and N = 3"""
    hw = [SHAPES[i % 2], SHAPES[2 + (i // 2) % 2], SHAPES[4]]
    return [((3, 1)[(i + pos) % 2],) + s_ for pos, s_ in enumerate(hw)]


CONV_PARAMS = [(cls, regime, shape) for i, cls in enumerate(CLASSES) for regime in ("int", "denorm", "cancel")
               for shape in shapes_of(i)]
CONV_PARAMS += [(cls, "overflow", shape) for i, cls in enumerate(CLASSES) if "overflow" in regimes_of(cls)
                for shape in shapes_of(i)]

# Every persistent kernel launches at most 8 XCDs x 32 = 256 workgroups (G = min(32, units per XCD)) and deals the units of
# an XCD round robin to its G workgroups.  With at least 3 x 256 = 768 units spread evenly over the XCDs every workgroup
# walks at least three of them: the halo and weight rings wrap and the residual prefetch two units ahead crosses units.
PERSISTENT_WORKGROUPS = 256


def walked(units):
    """asserts the rule above for a lower bound of a launch's units"""
    assert units >= 3 * PERSISTENT_WORKGROUPS, "%d units: not every workgroup walks three" % units


def conv_units(cls, shape):
    """a lower bound of the units of a persistent conv launch, whatever tile the launch code picks"""
    cin, cout, k, s = cls
    N, Ho, Wo = shape
    if cls == (64, 64, 3, 1):               # conv64.hip: 16 x 16 tiles, one cout block
        return N * -(-Ho // 16) * -(-Wo // 16)
    if cin == 48 and s == 2:                # conv48s2.hip: 8 x 8 output tiles, >= 1 cout block
        return N * -(-Ho // 8) * -(-Wo // 8)
    # conv_stream.hip: at least one tile per image whatever the tile candidate, and cout blocks of at most 48 channels
    # (conv_stream_supports: mt <= 3 at stride 1)
    return N * (cout // 48)


MANY_UNITS = [
    # conv_stream: 9 x 17 maps (a pixel over the 8 x 16 candidate, inside the larger ones), N = 768 / (cout / 48)
    ((48, 48, 3, 1), "denorm", (768, 9, 17)),        # >= 768 tiles x 1 cout block
    ((96, 96, 3, 1), "cancel", (384, 9, 17)),        # >= 384 tiles x 2 cout blocks = 768
    ((192, 192, 3, 1), "denorm", (192, 9, 17)),      # >= 192 tiles x 4 cout blocks = 768
    ((384, 384, 3, 1), "cancel", (96, 9, 17)),       # >= 96 tiles x 8 cout blocks = 768
    ((64, 64, 3, 1), "denorm", (200, 17, 33)),       # conv64: 200 x 2 x 3 tiles of 16 x 16 = 1,200
    ((48, 48, 3, 2), "denorm", (11, 68, 68)),        # conv48s2: 11 x 9 x 9 tiles of 8 x 8 = 891 units
    ((48, 96, 3, 2), "cancel", (11, 68, 68)),        # 891 units (two cout groups per workgroup)
    ((48, 384, 3, 2), "int", (11, 68, 68)),          # 891 tiles x 2 cout blocks (four cout groups per workgroup) = 1,782
]


def _CID(v):
    """test ids: a layer class, a (N, H, W) shape, or the value itself"""
    if isinstance(v, tuple):
        return {3: "n%d_%dx%d", 4: "%d-%d_k%ds%d", 5: "%d-%d_k%ds%dd%d"}[len(v)] % v
    return str(v)



def _run_conv_case(nat, cls, regime, shape, every_flag=True):
    cin, cout, k, s = cls
    N, Ho, Wo = shape
    H, W = Ho * s, Wo * s
    has_res, has_relu = class_flags(cls)
    L = nat.lib()
    st = nat.stream_ptr(torch.device(DEV))
    base = exact.exact_case(cin, cout, k, s, 1, N, H, W, regime, seed_of(cls, regime, shape), True, False, True)
    xg = exact.guarded(_nhwc(base.x), exact.IN_SENTINEL)
    rg = exact.guarded(_nhwc(base.res), exact.IN_SENTINEL)
    wn, a_np, b_np = base.w.contiguous().numpy(), base.alpha.numpy(), base.beta.numpy()
    launches = 0
    for round_conv in ((1, 0) if every_flag else (1,)):
        for use_res in ((1, 0) if has_res and every_flag else (int(has_res),)):
            for relu in ((1, 0) if has_relu and every_flag else (int(has_relu),)):
                c = exact.exact_case(cin, cout, k, s, 1, N, H, W, regime, seed_of(cls, regime, shape), bool(use_res),
                                     bool(relu), bool(round_conv))
                want = _nhwc(c.want).numpy()
                if round_conv:
                    _check_regime(regime, c)
                flags = (nat.F_RELU if relu else 0) | (nat.F_ROUND_CONV if round_conv else 0)
                for opts in class_options(cls):
                    yg = exact.guarded_out((N, Ho, Wo, cout), torch.float16)
                    with _Options(nat, **opts):
                        nat.check(L.rtpe_conv2d_nhwc(xg.t.data_ptr(), N, H, W, cin, wn.ctypes.data, a_np.ctypes.data_as(FPT),
                                                     b_np.ctypes.data_as(FPT), cout, k, s, flags,
                                                     rg.t.data_ptr() if use_res else None, yg.t.data_ptr(), st))
                    launches += 1
                    what = "conv %s %s n%d %dx%d round_conv=%d res=%d relu=%d %s" % (cls, regime, N, Ho, Wo, round_conv,
                                                                                     use_res, relu, opts)
                    _same(yg.t.cpu().numpy(), want, what)
                    assert exact.guards_intact(xg, rg, yg), what
    return launches


def _check_regime(regime, c):
    """the case reaches what its regime claims"""
    out = c.want.float()
    if regime == "denorm":          # denormal inputs, normal-range results (looked at in front of the ReLU)
        assert float(c.x.float().abs().max()) < 2.0 ** -14
        assert (c.ref.bn.abs() >= 2.0 ** -14).double().mean().item() > 0.9
    if regime == "cancel":
        assert torch.isfinite(out).all()
    if regime == "overflow":
        assert torch.isinf(out).any() and torch.isfinite(out).any() and not torch.isnan(out).any()


@pytest.mark.parametrize("cls,regime,shape", CONV_PARAMS, ids=_CID)
def test_conv2d_is_exact(nat, cls, regime, shape):
    """rtpe_conv2d_nhwc: every (cin, cout, k, stride) of CONV_CASES x regime x F_ROUND_CONV on / off x residual and ReLU
    on / off where the class has them, under each setting of tile_dma and of the class's own variant switch (direct_1x1,
    conv64, conv48s2)"""
    n = _run_conv_case(nat, cls, regime, shape)
    print("%d launches" % n)


@pytest.mark.parametrize("cls,regime,shape", MANY_UNITS, ids=_CID)
def test_conv2d_is_exact_with_more_units_than_workgroups(nat, cls, regime, shape):
    """the persistent kernels (conv_stream at 48 / 96 / 192 / 384, conv64, conv48s2) where a workgroup walks several units;
    with the layer's own flags (the small shapes walk every combination), under every option setting"""
    walked(conv_units(cls, shape))
    _run_conv_case(nat, cls, regime, shape, every_flag=False)


# --------------------------------------------------------------------------- #
# rtpe_basicblock_nhwc
# --------------------------------------------------------------------------- #
# the producer / consumer kernel takes H % 8 == 0 and W % 16 == 0 (8 x 16 tiles); everything else runs the resident-weights
# kernel (6 x 32 tiles); conv_block_supports wants H >= 6 and W >= 16.  (5, 70, 100) is ragged with several tiles per image
# (240 tiles: one per workgroup); BLOCK_MANY has 24 x 6 x 8 = 1,152 tiles of 8 x 16 and 24 x 8 x 4 = 768 of 6 x 32.
BLOCK_MANY = (24, 48, 128)
BLOCK_SHAPES = [(1, 8, 16), (3, 16, 32), (1, 9, 17), (3, 7, 33), (1, 6, 16), (1, 23, 37), (5, 70, 100), BLOCK_MANY]


@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=lambda s: "n%d_%dx%d" % s)
def test_basicblock_is_exact(nat, shape):
    N, H, W = shape
    L = nat.lib()
    st = nat.stream_ptr(torch.device(DEV))
    if shape == BLOCK_MANY:
        walked(min(N * (H // 8) * (W // 16), N * -(-H // 6) * -(-W // 32)))
    b = exact.exact_block(N, H, W, SEED + H * 100 + W)
    assert float(b.mid.float().max()) < 512
    xg = exact.guarded(_nhwc(b.x), exact.IN_SENTINEL)
    want = _nhwc(b.want).numpy()
    w1, w2 = b.w1.contiguous().numpy(), b.w2.contiguous().numpy()
    ab = [t.numpy() for t in (b.alpha1, b.beta1, b.alpha2, b.beta2)]
    for pc in (0, 1):
        for ring in (0, 1):
            yg = exact.guarded_out((N, H, W, 48), torch.float16)
            with _Options(nat, block_pc=pc, block_ring=ring):
                nat.check(L.rtpe_basicblock_nhwc(xg.t.data_ptr(), N, H, W, w1.ctypes.data, ab[0].ctypes.data_as(FPT),
                                                 ab[1].ctypes.data_as(FPT), w2.ctypes.data, ab[2].ctypes.data_as(FPT),
                                                 ab[3].ctypes.data_as(FPT), yg.t.data_ptr(), st))
            what = "basic block n%d %dx%d block_pc=%d block_ring=%d" % (N, H, W, pc, ring)
            _same(yg.t.cpu().numpy(), want, what)
            assert exact.guards_intact(xg, yg), what
    # the same block as two layer launches: the intermediate is THE intermediate
    mg = exact.guarded_out((N, H, W, 48), torch.float16)
    nat.check(L.rtpe_conv2d_nhwc(xg.t.data_ptr(), N, H, W, 48, w1.ctypes.data, ab[0].ctypes.data_as(FPT),
                                 ab[1].ctypes.data_as(FPT), 48, 3, 1, nat.F_RELU | nat.F_ROUND_CONV, None, mg.t.data_ptr(), st))
    _same(mg.t.cpu().numpy(), _nhwc(b.mid).numpy(), "first layer of the block n%d %dx%d" % shape)
    assert exact.guards_intact(xg, mg)


# --------------------------------------------------------------------------- #
# rtpe_deconv4x4s2_nhwc
# --------------------------------------------------------------------------- #
# input sizes; deconv48.hip's tile is 8 x 16 input positions.  The last one has 200 x 2 x 2 = 800 tiles.
DECONV_SHAPES = [(3, 3, 5), (1, 5, 7), (1, 9, 17), (3, 17, 33), (1, 23, 37), (200, 9, 17)]
DECONV_PARAMS = [(cin, regime, shape) for cin in (48, 96) for regime in ("int", "denorm", "cancel")
                 for shape in DECONV_SHAPES[:5]] + [(96, "denorm", DECONV_SHAPES[5]), (48, "cancel", DECONV_SHAPES[5])]


@pytest.mark.parametrize("cin,regime,shape", DECONV_PARAMS, ids=_CID)
def test_deconv_is_exact(nat, cin, regime, shape):
    N, H, W = shape
    L = nat.lib()
    st = nat.stream_ptr(torch.device(DEV))
    seed = SEED + cin + H * 100 + W + exact.REGIMES.index(regime)
    base = exact.exact_case(cin, 48, 4, 2, 1, N, H, W, regime, seed, False, False, True, transposed=True)
    xg = exact.guarded(_nhwc(base.x), exact.IN_SENTINEL)
    wn, a_np, b_np = base.w.contiguous().numpy(), base.alpha.numpy(), base.beta.numpy()
    small = N * H * W < 20000                # the large case: the layer's own flags only
    if not small:
        walked(N * -(-H // 8) * -(-W // 16))
    for round_conv in ((1, 0) if small else (1,)):
        for relu in ((1, 0) if small else (1,)):
            c = exact.exact_case(cin, 48, 4, 2, 1, N, H, W, regime, seed, False, bool(relu), bool(round_conv), transposed=True)
            if round_conv:
                _check_regime(regime, c)
            want = _nhwc(c.want).numpy()
            for on in (0, 1):
                for dma in (0, 1):
                    yg = exact.guarded_out((N, 2 * H, 2 * W, 48), torch.float16)
                    with _Options(nat, deconv48=on, tile_dma=dma):
                        nat.check(L.rtpe_deconv4x4s2_nhwc(xg.t.data_ptr(), N, H, W, cin, wn.ctypes.data, a_np.ctypes.data_as(FPT),
                                                          b_np.ctypes.data_as(FPT), 48,
                                                          (nat.F_RELU if relu else 0) | (nat.F_ROUND_CONV if round_conv else 0),
                                                          yg.t.data_ptr(), st))
                    what = "deconv %d->48 %s n%d %dx%d round_conv=%d relu=%d deconv48=%d tile_dma=%d" % (
                        cin, regime, N, H, W, round_conv, relu, on, dma)
                    _same(yg.t.cpu().numpy(), want, what)
                    assert exact.guards_intact(xg, yg), what


# --------------------------------------------------------------------------- #
# rtpe_conv2d_nhwc_ex with F_F32
# --------------------------------------------------------------------------- #
F32_PARAMS = [(cls, shape) for i, cls in enumerate(F32_CLASSES) for shape in shapes_of(i)]


@pytest.mark.parametrize("cls,shape", F32_PARAMS, ids=_CID)
def test_conv2d_fp32_is_exact(nat, cls, shape):
    """the fp32 kernels (v_mfma_f32_16x16x4_f32; dilations 1, 2, 3, 5 and the 5x5 stride-2 conv) on integer data that stays
    below 2^24 through BatchNorm and the add: no rounding anywhere, one right answer"""
    cin, cout, k, s, dil = cls
    N, Ho, Wo = shape
    H, W = Ho * s, Wo * s
    L = nat.lib()
    st = nat.stream_ptr(torch.device(DEV))
    seed = SEED + cin * 3 + cout + dil + Ho
    base = exact.exact_case(cin, cout, k, s, dil, N, H, W, "int", seed, True, False, False, f32=True)
    xg = exact.guarded(_nhwc(base.x), exact.IN_SENTINEL)
    rg = exact.guarded(_nhwc(base.res), exact.IN_SENTINEL)
    wn, a_np, b_np = base.w.contiguous().numpy(), base.alpha.numpy(), base.beta.numpy()
    for use_res in (1, 0):
        for relu in (1, 0):
            c = exact.exact_case(cin, cout, k, s, dil, N, H, W, "int", seed, bool(use_res), bool(relu), False, f32=True)
            want = _nhwc(c.want).numpy()
            for dma in (0, 1):
                yg = exact.guarded_out((N, Ho, Wo, cout), torch.float32)
                with _Options(nat, tile_dma=dma):
                    nat.check(L.rtpe_conv2d_nhwc_ex(xg.t.data_ptr(), N, H, W, cin, wn.ctypes.data, a_np.ctypes.data_as(FPT),
                                                    b_np.ctypes.data_as(FPT), cout, k, s, dil,
                                                    (nat.F_RELU if relu else 0) | nat.F_F32,
                                                    rg.t.data_ptr() if use_res else None, yg.t.data_ptr(), st))
                what = "fp32 conv %s n%d %dx%d res=%d relu=%d tile_dma=%d" % (cls, N, Ho, Wo, use_res, relu, dma)
                _same(yg.t.cpu().numpy(), want, what)
                assert exact.guards_intact(xg, rg, yg), what


# --------------------------------------------------------------------------- #
# programs: stem (+ the 64 -> 64 stride-2 conv behind it), the direct heads, the 1x1 pair
# --------------------------------------------------------------------------- #
def _forward(nat, eng, xg, N, H, W, out_shapes, op_ms=None):
    """rtpe_hrnet_forward on guarded input and outputs (the workspace is the executor's own); ``op_ms``: a list that
    receives the per-op times of rtpe_hrnet_forward_timed instead"""
    ws = eng.workspace(N, H, W)
    pg, rg = [exact.guarded_out(s_, torch.float32) for s_ in out_shapes]
    xdt = nat.RTPE_DTYPE_F16 if xg.t.dtype == torch.float16 else nat.RTPE_DTYPE_F32
    args = (eng._h, xg.t.data_ptr(), xdt, N, H, W, pg.t.data_ptr(), rg.t.data_ptr(), nat.RTPE_DTYPE_F32, ws.data_ptr(),
            ws.numel(), nat.stream_ptr(torch.device(DEV)))
    if op_ms is None:
        nat.check(nat.lib().rtpe_hrnet_forward_flags(*args, 0))
    else:
        ms = (ctypes.c_float * len(eng.program.ops))()
        nat.check(nat.lib().rtpe_hrnet_forward_timed(*args, ms, len(ms)))
        op_ms[:] = list(ms)
    torch.cuda.synchronize()
    return pg, rg


def _affine_is_exact(layer):
    from rtpe.third_party.pose_higher_hrnet import ProgramBuilder
    conv, norm, w, alpha, beta = layer
    ab = np.frombuffer(ProgramBuilder._affine(conv, norm, conv.out_channels), dtype=np.float32)
    return np.array_equal(ab, torch.cat([alpha, beta]).float().numpy())


# input sizes (multiples of 32): the heads sit at 1/8.  The direct head kernel takes maps whose pixel count per image is a
# multiple of 32 (conv_head_supports): 32 (3 wave steps of 32 pixels, one workgroup), 128 and 512 (2 x 512 pixels = 32 steps:
# several workgroups); the maps of 16, 48 and 240 pixels stay on the tile kernel under either setting.  The test asserts
# which kernel runs.  (The direct kernel's loop over steps starts beyond 2,048 workgroups: not reached at test sizes.)
STEM_SHAPES = [(1, 32, 32, "f16"), (3, 64, 32, "f32"), (2, 96, 32, "inexact"), (1, 96, 160, "inexact"), (2, 128, 64, "f32"),
               (2, 256, 128, "inexact")]


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "n%d_%dx%d_%s" % s)
def test_stem_and_direct_heads_are_exact(nat, shape):
    """stem + 64 -> 64 stride-2 conv (fused_stem 0 / 1 / 2), a 64 -> 48 stride-2 conv and the 48 -> 34 / 48 -> 17 heads with
    bias and fp32 NCHW output (head_direct 0 / 1).  Input: fp16, fp32 whose .half() is exact, and fp32 that is NOT an fp16
    number (x * (1 + 2^-13): the load-time rounding to fp16 is part of the reference)."""
    from rtpe.third_party.pose_higher_hrnet import Engine, ProgramBuilder
    N, H, W, kind = shape
    g = torch.Generator().manual_seed(SEED + H + W)
    stem, conv2, conv3 = _layer(3, 64, 3, 2, g), _layer(64, 64, 3, 2, g), _layer(64, 48, 3, 2, g)
    heads = [_layer(48, 34, 1, 1, g, bn=False), _layer(48, 17, 1, 1, g, bn=False)]
    assert all(_affine_is_exact(l) for l in [stem, conv2, conv3] + heads)
    b = ProgramBuilder(f32=False)
    t = b.stem(stem[0], stem[1])
    t = b.conv(t, conv2[0], conv2[1], relu=True)
    t = b.conv(t, conv3[0], conv3[1], relu=True)
    b.conv(t, heads[0][0], None, out_flag=nat.F_OUT_PREDS, nhwc=False)
    b.conv(t, heads[1][0], None, out_flag=nat.F_OUT_REFINED, nhwc=False)
    eng = Engine(b.finish(), 0)
    xi = torch.randint(-3, 4, (N, 3, H, W), generator=g).float()
    x = {"f16": xi.half(), "f32": xi, "inexact": xi * (1 + 2.0 ** -13)}[kind]
    if kind == "inexact":
        assert not torch.equal(x.half().float(), x) and torch.equal(x.half().float(), xi)
    y = _ref_layer(x.half().double(), stem, 3, 2, True, True, quantum=1.0)
    y = _ref_layer(y, conv2, 3, 2, True, True, quantum=0.5)
    y = _ref_layer(y, conv3, 3, 2, True, True, quantum=0.25)
    want = [_ref_layer(y, hd, 1, 1, False, False, quantum=0.125).float().numpy() for hd in heads]
    xg = exact.guarded(x, exact.IN_SENTINEL)
    shapes = [(N, 34, H // 8, W // 8), (N, 17, H // 8, W // 8)]
    for fused in (0, 1, 2):
        for direct in (0, 1):
            with _Options(nat, fused_stem=fused, head_direct=direct):
                takes = (H // 8) * (W // 8) % 32 == 0
                assert [eng.op_tile(i, N, H, W)[7] == -400001 for i in (3, 4)] == [takes and direct == 1] * 2
                if fused != 2:
                    assert (eng.op_tile(0, N, H, W)[7] == -600001) == (fused == 1)
                pg, rg = _forward(nat, eng, xg, N, H, W, shapes)
            what = "stem program n%d %dx%d %s fused_stem=%d head_direct=%d" % (N, H, W, kind, fused, direct)
            _same(pg.t.cpu().numpy(), want[0], what + " head 34")
            _same(rg.t.cpu().numpy(), want[1], what + " head 17")
            assert exact.guards_intact(xg, pg, rg), what


def _block_program(g):
    """the layers of: stem, conv 3x3 64 -> 48 stride 2 (the map at 1/4), one BasicBlock of the 48-channel branch (which
    the executor flags for conv_block.hip), the two heads.  One alpha per layer behind the stem and a quarter of the
    block's weights: max |activation| / quantum grows by about sqrt(taps x density) per layer, and the last sums
    (48 taps at quantum 1/16) must stay below 2^24 quanta - _ref_layer asserts it for every layer of the chain"""
    stem = _layer(3, 64, 3, 2, g)
    down = _layer(64, 48, 3, 2, g, alpha_choices=(0.5,), density=0.5)
    c1 = _layer(48, 48, 3, 1, g, alpha_choices=(0.5,), density=0.25)
    c2 = _layer(48, 48, 3, 1, g, alpha_choices=(0.5,), density=0.25)
    heads = [_layer(48, 34, 1, 1, g, bn=False), _layer(48, 17, 1, 1, g, bn=False)]
    return stem, down, c1, c2, heads


def _block_program_reference(layers, x):
    stem, down, c1, c2, heads = layers
    y = _ref_layer(x.double(), stem, 3, 2, True, True, quantum=1.0)
    y = _ref_layer(y, down, 3, 2, True, True, quantum=0.5)
    m = _ref_layer(y, c1, 3, 1, True, True, quantum=0.25)
    y = _ref_layer(m, c2, 3, 1, True, True, res=y, quantum=0.125)
    return [_ref_layer(y, hd, 1, 1, False, False, quantum=0.0625).float().numpy() for hd in heads]


# input sizes: the block's map is the input's quarter.  conv_block_supports takes maps from 6 x 16 up: 16 x 16 and (W at
# its limit, N = 3) 8 x 16 fuse, 16 x 8 does not and runs the two convs as launches of their own
BLOCK_PROGRAM_SHAPES = [(1, 64, 64, True), (1, 64, 32, False), (3, 32, 64, True)]


@pytest.mark.parametrize("shape", BLOCK_PROGRAM_SHAPES, ids=lambda s: "n%d_%dx%d_%s" % (s[:3] + ("fused" if s[3] else "two_launches",)))
def test_basicblock_in_a_program_is_labelled_and_timed_as_it_runs(nat, shape):
    """A flagged BasicBlock at a map size the fused kernel takes and at one it does not: rtpe_hrnet_op_tile and the per-op
    times of rtpe_hrnet_forward_timed say what ran (the fused kernel: marks -900001 / -900002, the second conv's time
    exactly 0; two launches: their launch shapes, a time each), and the outputs are THE answer either way."""
    from rtpe.third_party.pose_higher_hrnet import Engine, ProgramBuilder
    N, H, W, fuses = shape
    g = torch.Generator().manual_seed(SEED + 48)
    layers = _block_program(g)
    stem, down, c1, c2, heads = layers
    assert all(_affine_is_exact(l) for l in [stem, down, c1, c2] + heads)
    b = ProgramBuilder(f32=False)
    t = b.stem(stem[0], stem[1])
    t = b.conv(t, down[0], down[1], relu=True)
    m = b.conv(t, c1[0], c1[1], relu=True)
    t = b.conv(m, c2[0], c2[1], relu=True, residual=t)
    b.conv(t, heads[0][0], None, out_flag=nat.F_OUT_PREDS, nhwc=False)
    b.conv(t, heads[1][0], None, out_flag=nat.F_OUT_REFINED, nhwc=False)
    eng = Engine(b.finish(), 0)
    # ops 2 and 3 are the block, and the executor flagged them: at a fusing size they report the fused kernel
    assert [eng.op_tile(i, 1, 64, 64)[7] for i in (2, 3)] == [-900001, -900002]
    x = torch.randint(-3, 4, (N, 3, H, W), generator=g).half()
    want = _block_program_reference(layers, x)
    xg = exact.guarded(x, exact.IN_SENTINEL)
    shapes = [(N, 34, H // 4, W // 4), (N, 17, H // 4, W // 4)]
    tiles = [eng.op_tile(i, N, H, W) for i in (2, 3)]
    ms = []
    _forward(nat, eng, xg, N, H, W, shapes, op_ms=ms)
    if fuses:
        assert [t_[7] for t_ in tiles] == [-900001, -900002]
        assert ms[2] > 0 and ms[3] == 0.0
    else:
        for t_ in tiles:                                  # a launch shape: pixel tiles, waves, a tile; LDS bytes or the streaming form
            assert t_[7] not in (-900001, -900002) and (t_[7] > 0 or t_[7] <= -100000)
            assert t_[0] > 0 and t_[1] > 0 and t_[2] > 0 and t_[3] > 0 and t_[4] > 0
        assert ms[2] > 0 and ms[3] > 0
    for fused in (0, 1):
        for direct in (0, 1):
            with _Options(nat, fused_stem=fused, head_direct=direct):
                pg, rg = _forward(nat, eng, xg, N, H, W, shapes)
            what = "block program n%d %dx%d fused_stem=%d head_direct=%d" % (N, H, W, fused, direct)
            _same(pg.t.cpu().numpy(), want[0], what + " head 34")
            _same(rg.t.cpu().numpy(), want[1], what + " head 17")
            assert exact.guards_intact(xg, pg, rg), what


@pytest.mark.parametrize("shape", [(1, 32, 32), (3, 64, 96), (2, 96, 160)], ids=lambda s: "n%d_%dx%d" % s)
def test_1x1_pair_is_exact(nat, shape):
    """conv 1x1 64 -> 256 + residual + ReLU and the conv 1x1 256 -> 64 + ReLU behind it, which the program compiler flags
    RTPE_F_PAIR_HEAD / _TAIL: as one kernel (pair_1x1 = 1, csrc/conv_pair.hip) and as two launches"""
    from rtpe.third_party.pose_higher_hrnet import Engine, ProgramBuilder
    N, H, W = shape
    g = torch.Generator().manual_seed(SEED + 3 * H + W)
    stem, skip = _layer(3, 64, 3, 2, g), _layer(64, 256, 1, 1, g)
    head, tail = _layer(64, 256, 1, 1, g), _layer(256, 64, 1, 1, g)
    outs = [_layer(64, 34, 1, 1, g, bn=False), _layer(64, 17, 1, 1, g, bn=False)]
    assert all(_affine_is_exact(l) for l in [stem, skip, head, tail] + outs)
    b = ProgramBuilder(f32=False)
    t64 = b.stem(stem[0], stem[1])
    t256 = b.conv(t64, skip[0], skip[1], relu=False)
    th = b.conv(t64, head[0], head[1], relu=True, residual=t256)
    tt = b.conv(th, tail[0], tail[1], relu=True)
    b.conv(tt, outs[0][0], None, out_flag=nat.F_OUT_PREDS, nhwc=False)
    b.conv(tt, outs[1][0], None, out_flag=nat.F_OUT_REFINED, nhwc=False)
    prog = b.finish()
    assert prog.ops[2].flags & nat.F_PAIR_HEAD and prog.ops[3].flags & nat.F_PAIR_TAIL
    eng = Engine(prog, 0)
    x = torch.randint(-3, 4, (N, 3, H, W), generator=g).half()
    y64 = _ref_layer(x.double(), stem, 3, 2, True, True, quantum=1.0)
    y256 = _ref_layer(y64, skip, 1, 1, False, True, quantum=0.5)
    yh = _ref_layer(y64, head, 1, 1, True, True, res=y256, quantum=0.5)
    yt = _ref_layer(yh, tail, 1, 1, True, True, quantum=0.25)
    want = [_ref_layer(yt, hd, 1, 1, False, False, quantum=0.125).float().numpy() for hd in outs]
    xg = exact.guarded(x, exact.IN_SENTINEL)
    shapes = [(N, 34, H // 2, W // 2), (N, 17, H // 2, W // 2)]
    for pair in (0, 1):
        with _Options(nat, pair_1x1=pair):
            pg, rg = _forward(nat, eng, xg, N, H, W, shapes)
        what = "1x1 pair program n%d %dx%d pair_1x1=%d" % (N, H, W, pair)
        _same(pg.t.cpu().numpy(), want[0], what + " head 34")
        _same(rg.t.cpu().numpy(), want[1], what + " head 17")
        assert exact.guards_intact(xg, pg, rg), what


# --------------------------------------------------------------------------- #
# sibling 3x3 stride-2 convs from one 48-channel map: conv48s2_launch_group, two or three layers as one grid
# --------------------------------------------------------------------------- #
S2_PREFIX = [3, 2, 4, 8, 8, 48]                     # rtpe_hrnet_op_tile of an op on conv48s2.hip, in front of n_cb and the mark
SIBLING_PARAMS = [(set_id, shape) for i, set_id in enumerate(host.SIBLING_IDS) for shape in host.sibling_shapes(i)]
SIBLING_PARAMS += [(set_id, host.SIBLING_WALKED) for set_id in host.SIBLING_WALKED_IDS]


def _selection_head(c):
    """a 1x1 conv without bias whose weights are the identity: output channel j is input channel j, exactly"""
    import torch.nn as nn
    conv = nn.Conv2d(c, c, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.eye(c).view(c, c, 1, 1))
    return conv.half()


def _sibling_engine(nat, set_id, deep, read):
    """the program of a sibling set: front, the siblings next to each other, and two heads that read the siblings
    ``read``; returns the executor and the index of the first sibling op"""
    from rtpe.third_party.pose_higher_hrnet import Engine, ProgramBuilder
    sibs = host.SIBLING_SETS[host.SIBLING_IDS.index(set_id)][1]
    stem, convs = host.sibling_front_layers(deep)
    layers = host.sibling_layers(set_id)
    assert all(_affine_is_exact(l) for l in [stem] + [c[0] for c in convs] + layers)
    b = ProgramBuilder(f32=False)
    t = b.stem(stem[0], stem[1])
    for layer, k, s in convs:
        t = b.conv(t, layer[0], layer[1], relu=True)
    first = len(b.ops)
    outs = [b.conv(t, l[0], l[1], relu=bool(c[1])) for l, c in zip(layers, sibs)]
    for k, flag in zip(read, (nat.F_OUT_PREDS, nat.F_OUT_REFINED)):
        b.conv(outs[k], _selection_head(sibs[k][0]), None, out_flag=flag, nhwc=False)
    prog = b.finish()
    assert [(d.cin, d.cout, d.ksize, d.stride, d.in_t) for d in prog.ops[first:first + len(sibs)]] == \
        [(48, c[0], 3, 2, t) for c in sibs]
    return Engine(prog, 0), first


@pytest.mark.parametrize("set_id,shape", SIBLING_PARAMS, ids=_CID)
def test_sibling_stride2_convs_are_exact_as_one_launch(nat, set_id, shape):
    """Two to four 3x3 stride-2 convs (48 or 96 output channels; each its own weights, alpha / beta, ReLU flag) that read
    the same 48-channel map next to each other in a program: the executor runs the runs its static rule forms as ONE
    launch of conv48s2.hip (conv48s2_launch_group: a slot per group of 48 channels with its own weights, affine, ReLU flag,
    destination and row pitch).  Every element of every sibling is read back through a 1x1 head with identity weights
    (fp32 NCHW; it reads -0 as +0: its sum starts at +0) - two siblings per program, so a set of three or four runs the
    same layers in two programs - and compared with the float64 reference of its own layer
    (test_conv_exact_host.sibling_outputs).  Asserted for every case: the launch labels under the default options (the
    group marks of include/rtpe_hip.h: a test that silently ran single launches would prove nothing) and with conv48s2 = 0
    (no conv48s2 mark), the per-op times of the small shapes, the outputs under conv48s2 0 / 1 x tile_dma 0 / 1, and the
    guard bands.  The workspace is refilled with a finite value in front of every forward, so that an element a launch
    does not write cannot keep the right value of the forward before."""
    i = host.SIBLING_IDS.index(set_id)
    sibs, marks = host.SIBLING_SETS[i][1:]
    N, Ho, Wo = shape
    deep = shape != host.SIBLING_WALKED
    if not deep:
        walked(N * (Ho // 8) * (Wo // 8))
        assert N * (Ho // 8) * (Wo // 8) >= 5 * PERSISTENT_WORKGROUPS        # a workgroup's fifth halo tile: the ring of 4 wraps
    x, t, q = host.sibling_front(deep, N, Ho, Wo)
    H, W = x.shape[2:]
    want = [(o + 0.0).float().numpy() for o in host.sibling_outputs(set_id, t, q)]
    xg = exact.guarded(x, exact.IN_SENTINEL)
    n = len(sibs)
    fill = int(torch.tensor([host.SIBLING_PRESET], dtype=torch.float16).view(torch.int16)[0])
    for read in [(0, 1)] + ([(2, 3 if n == 4 else 0)] if n > 2 else []):
        eng, first = _sibling_engine(nat, set_id, deep, read)
        ops = range(first, first + n)
        shapes = [(N, sibs[k][0], Ho, Wo) for k in read]

        def forward(what, **kw):
            eng.workspace(N, H, W).view(torch.int16).fill_(fill)
            pg, rg = _forward(nat, eng, xg, N, H, W, shapes, **kw)
            _same(pg.t.cpu().numpy(), want[read[0]], what + " sibling %d" % read[0])
            _same(rg.t.cpu().numpy(), want[read[1]], what + " sibling %d" % read[1])
            assert exact.guards_intact(xg, pg, rg), what

        what = "siblings %s n%d %dx%d heads %s" % (set_id, N, Ho, Wo, read)
        assert [eng.op_tile(op, N, H, W) for op in ops] == [S2_PREFIX + [1, m] for m in marks], what
        if deep:
            # the first op of a group and a conv on its own are launches; an op the group's launch computes has an event of
            # its own behind the group's with no kernel between them (include/rtpe_hip.h, rtpe_hrnet_forward_timed)
            ms = []
            forward(what + " timed", op_ms=ms)
            for op, m in zip(ops, marks):
                assert np.isfinite(ms[op]) and (ms[op] >= 0.0 if m == -200009 else ms[op] > 0.0), (what, op, m, ms[op])
        for s2 in (1, 0):
            for dma in (0, 1):
                with _Options(nat, conv48s2=s2, tile_dma=dma):
                    tiles = [eng.op_tile(op, N, H, W) for op in ops]
                    if s2:
                        assert [t_[7] for t_ in tiles] == marks, (what, tiles)
                    else:
                        assert not any(t_[:6] == S2_PREFIX and -200010 < t_[7] <= -200001 for t_ in tiles), (what, tiles)
                    forward(what + " conv48s2=%d tile_dma=%d" % (s2, dma))


# --------------------------------------------------------------------------- #
# rtpe_fuse_nhwc
# --------------------------------------------------------------------------- #
def _fuse_case(nat, N, H, W, C, n_terms, f32, relu, seed):
    dt = torch.float32 if f32 else torch.float16
    g = torch.Generator().manual_seed(seed)
    ups = list(range(n_terms))
    terms = [torch.randn(N, H >> u, W >> u, C, generator=g).to(dt) for u in ups]
    want = terms[0].clone()
    for t, u in zip(terms[1:], ups[1:]):
        up = t.repeat_interleave(1 << u, dim=1).repeat_interleave(1 << u, dim=2)      # nearest upsampling
        want = want + up                                                                # one rounding per add
    if relu:
        want = F.relu(want)
    tg = [exact.guarded(t, exact.IN_SENTINEL) for t in terms]
    yg = exact.guarded_out((N, H, W, C), dt)
    ptrs = (ctypes.c_void_p * 4)(*([t.t.data_ptr() for t in tg] + [None] * (4 - n_terms)))
    upa = (ctypes.c_int32 * 4)(*(ups + [0] * (4 - n_terms)))
    nat.check(nat.lib().rtpe_fuse_nhwc(ptrs, upa, n_terms, N, H, W, C, (nat.F_RELU if relu else 0) | (nat.F_F32 if f32 else 0),
                                       yg.t.data_ptr(), nat.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    what = "fuse n%d %dx%d C=%d terms=%d f32=%d relu=%d" % (N, H, W, C, n_terms, f32, relu)
    _same(yg.t.cpu().numpy(), want.numpy(), what)
    assert exact.guards_intact(yg, *tg), what


@pytest.mark.parametrize("C", [48, 96, 192, 384])
@pytest.mark.parametrize("f32", [0, 1], ids=["fp16", "fp32"])
def test_fuse_is_exact(nat, C, f32):
    """the fuse sum (each add is one IEEE rounding of an exact sum: bit-exact on any data), 1 - 4 terms with nearest
    upsampling, with and without the final ReLU, at a ragged size"""
    for n_terms in (1, 2, 3, 4):
        _fuse_case(nat, 3, 24, 40, C, n_terms, f32, n_terms % 2, SEED + C + n_terms)


def test_fuse_is_exact_beyond_one_grid_row_index(nat):
    """N * H = 65,544 output rows: more than the 65,535 a grid's y index holds, so the launch takes the grid-stride kernel
    instead of the one-workgroup-row-per-output-row kernel that every other shape in the suite runs"""
    _fuse_case(nat, 8193, 8, 8, 48, 2, 0, 1, SEED)
    _fuse_case(nat, 8193, 8, 8, 48, 2, 1, 0, SEED + 1)
