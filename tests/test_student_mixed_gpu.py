"""One forward over images of different sizes (include/rtpe_hip_mixed.h), on an MI355X (run with -m gpu).

Per op (tests 1xx): small ``any_size`` programs, fed through the stem (a mixed batch takes no second input).  Each program
runs once on a mixed batch - the three images of ``M.OP_SIZES`` in a canvas that is NaN outside every image - through the
C entry, with the canvas, both outputs and the workspace between guard bands, the outputs preset to a NaN pattern and the
workspace to a finite sentinel; and once per image alone through ``rtpe_hrnet_forward_flags``.  Image n's region of either
output must hold the bits of the image alone (``array_equal`` on the bit patterns), everything outside the regions must
be 0.0.  No tolerance anywhere: a mixed forward computes every pixel of an image with the operations, and in the order, of
the forward of that image alone.  Two canvases: 64 x 47, where every image reaches one canvas edge, and 72 x 80, where
none does and a whole tile row and column lie outside every image.

Whole network (2xx), ``StudentPipeline.call_mixed`` (3xx) and the refusals of the C side (4xx) below."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import test_student_mixed_host as M
import test_student_sizes_host as S
from oracle import exact, synth
from test_student_ops_gpu import _ws_guarded
from test_student_pipeline_gpu import _det, _n_people, _parser
from test_student_pipeline_gpu import _same as _same_people

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
J = 17


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


# --------------------------------------------------------------------------- #
# programs and the two runs
# --------------------------------------------------------------------------- #
def _gen(*key):
    return torch.Generator().manual_seed(77003 + sum((i + 1) * 257 * int(k) for i, k in enumerate(key)))


def _conv(g, cin, cout, k=3, s=1, d=1, bn=True, ints=False, positive=False):
    """Conv2d [+ BatchNorm2d] with seeded weights that are fp16 numbers (the same layer in an fp16 and an fp32 program);
    ``ints``: weights in {-1, 0, 1}, alpha 1, integer beta (sums that are exact in any order on integer data);
    ``positive``: weights in [1/16, 1) - positive inputs stay positive, no ReLU clips them"""
    conv = nn.Conv2d(cin, cout, k, s, d * (k // 2), d, bias=not bn)
    shape = conv.weight.shape
    if ints:
        w = torch.randint(-1, 2, shape, generator=g).float()
    elif positive:
        w = (torch.randint(1, 16, shape, generator=g).float() / 16) / (cin * k * k / 4.0)
    else:
        w = (torch.randn(shape, generator=g) / (cin * k * k) ** 0.5)
    norm = None
    with torch.no_grad():
        conv.weight.copy_(w.half().float())
        beta = torch.randint(-4, 5, (cout,), generator=g).float() / (1 if ints else 8)
        if positive:
            beta = beta.abs()
        if bn:
            norm = nn.BatchNorm2d(cout)
            alpha = torch.ones(cout) if ints else torch.randint(4, 9, (cout,), generator=g).float() / 8
            norm.weight.copy_(alpha); norm.bias.copy_(beta); norm.running_mean.zero_(); norm.running_var.fill_(1.0 - norm.eps)
        else:
            conv.bias.copy_(beta)
    return conv, norm


class Prog:
    """a ProgramBuilder with the any_size property and the shapes (channels, ds) of its two NCHW outputs"""

    def __init__(self, f32, granule=None):
        from rtpe.third_party.pose_higher_hrnet import ProgramBuilder
        self.b = ProgramBuilder(f32=f32, any_size=True, granule=(4 if f32 else 8) if granule is None else granule)
        self.shapes = [None, None]

    def head(self, nat, t, cout, which, g, k=1):
        conv, _ = _conv(g, self.b.tensors[t][0], cout, k, bn=False)
        self.b.conv(t, conv, None, out_flag=(nat.F_OUT_PREDS, nat.F_OUT_REFINED)[which], nhwc=False)
        self.shapes[which] = (cout, self.b.tensors[t][1])


def _engine(prog):
    from rtpe.third_party.pose_higher_hrnet import Engine
    p = prog.b.finish()
    assert p.any_size is True and not getattr(p, "has_aux", False)
    return Engine(p, 0)


def _images(sizes, g, ints=False, positive=False):
    if ints:
        return [torch.randint(-3, 4, (3, h, w), generator=g).float() for h, w in sizes]
    return [torch.rand(3, h, w, generator=g) + (0.5 if positive else -0.5) for h, w in sizes]


def _nan_canvas(images, canvas_hw):
    canvas = torch.full((len(images), 3) + tuple(canvas_hw), float("nan"))
    for n, im in enumerate(images):
        canvas[n, :, :im.shape[1], :im.shape[2]] = im
    return canvas


def _pinned(n):
    return torch.zeros(n, dtype=torch.int32).pin_memory()


def _forward_mixed_raw(nat, eng, shapes, canvas, sizes, expect_error=False):
    """rtpe_hrnet_forward_mixed on guarded buffers -> the two output canvases (numpy), or the return code"""
    L = nat.lib()
    N, _, Hc, Wc = canvas.shape
    xg = exact.guarded(canvas.contiguous(), exact.IN_SENTINEL)
    outs = []
    for s_ in shapes:
        shape = (N, s_[0], nat.extent(Hc, s_[1]), nat.extent(Wc, s_[1])) if s_ else (1, 1, 1, 64)
        outs.append(exact.guarded_out(shape, torch.float32))
    need = ctypes.c_size_t(1 << 20)
    rc_ws = L.rtpe_hrnet_mixed_workspace_bytes(eng._h, N, Hc, Wc, ctypes.byref(need))
    assert expect_error or rc_ws == 0
    wg = _ws_guarded(max(need.value, 256))
    n_ints = ctypes.c_int32()
    nat.check(L.rtpe_mixed_table_ints(N, ctypes.byref(n_ints)))
    table = _pinned(n_ints.value)
    flat = (ctypes.c_int32 * (2 * N))(*[v for hw in sizes for v in hw])
    xdt = nat.RTPE_DTYPE_F16 if canvas.dtype == torch.float16 else nat.RTPE_DTYPE_F32
    rc = L.rtpe_hrnet_forward_mixed(eng._h, xg.t.data_ptr(), xdt, N, Hc, Wc, flat, table.data_ptr(), table.numel(),
                                    outs[0].t.data_ptr(), outs[1].t.data_ptr(), nat.RTPE_DTYPE_F32, wg.t.data_ptr(),
                                    wg.t.numel() * 4, nat.stream_ptr(torch.device(DEV)), 0)
    torch.cuda.synchronize()
    assert exact.guards_intact(xg, outs[0], outs[1], wg), "a guard band was overwritten"
    if expect_error:
        for o in outs:                               # refused before the first launch: nothing was written
            assert rc == 0 or bool((o.t.view(torch.int32) == o.bits).all())
        return rc
    nat.check(rc)
    return [o.t.cpu().numpy() for o in outs]


def _forward_alone_raw(nat, eng, shapes, x):
    """the existing entry on one image (1, 3, h, w), guarded the same way"""
    L = nat.lib()
    _, _, H, W = x.shape
    xg = exact.guarded(x.contiguous(), exact.IN_SENTINEL)
    outs = []
    for s_ in shapes:
        shape = (1, s_[0], nat.extent(H, s_[1]), nat.extent(W, s_[1])) if s_ else (1, 1, 1, 64)
        outs.append(exact.guarded_out(shape, torch.float32))
    need = ctypes.c_size_t()
    nat.check(L.rtpe_hrnet_workspace_bytes(eng._h, 1, H, W, ctypes.byref(need)))
    wg = _ws_guarded(max(need.value, 256))
    nat.check(L.rtpe_hrnet_forward_flags(eng._h, xg.t.data_ptr(), nat.RTPE_DTYPE_F32, 1, H, W, outs[0].t.data_ptr(),
                                         outs[1].t.data_ptr(), nat.RTPE_DTYPE_F32, wg.t.data_ptr(), wg.t.numel() * 4,
                                         nat.stream_ptr(torch.device(DEV)), 0))
    torch.cuda.synchronize()
    assert exact.guards_intact(xg, outs[0], outs[1], wg), "a guard band was overwritten"
    return [o.t.cpu().numpy() for o in outs]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_regions(nat, got, alone, shapes, sizes, what):
    """image n's region of either output canvas holds the bits of the image alone; everything else is exactly 0.0"""
    for k, s_ in enumerate(shapes):
        rest = got[k].copy()
        for n, (h, w) in enumerate(sizes):
            eh, ew = nat.extent(h, s_[1]), nat.extent(w, s_[1])
            want = alone[n][k][0]
            assert want.shape == (s_[0], eh, ew) and np.isfinite(want).all(), (what, k, n, want.shape)
            region = got[k][n, :, :eh, :ew]
            assert np.array_equal(_bits(region), _bits(want)), \
                "%s: output %d, image %d (%d x %d): %s" % (what, k, n, h, w, exact.first_differences(region, want))
            rest[n, :, :eh, :ew] = 0
        assert np.array_equal(_bits(rest), np.zeros_like(_bits(rest))), \
            "%s: output %d holds %d elements that are not 0.0 outside the images" % (what, k, int((_bits(rest) != 0).sum()))
    return alone


def _mixed_vs_alone(nat, prog, canvas_hw, g, what, ints=False, positive=False, sizes=M.OP_SIZES):
    eng = _engine(prog)
    images = _images(sizes, g, ints, positive)
    got = _forward_mixed_raw(nat, eng, prog.shapes, _nan_canvas(images, canvas_hw), sizes)
    alone = [_forward_alone_raw(nat, eng, prog.shapes, im[None]) for im in images]
    for a in alone:                                 # the data reach the outputs: a mask that zeroes too much would show
        assert all(float(np.abs(o).max()) > 0 for o in a), what
    return _check_regions(nat, got, alone, prog.shapes, sizes, "%s in a %d x %d canvas" % ((what,) + tuple(canvas_hw)))


CANVAS = pytest.mark.parametrize("canvas_hw", M.OP_CANVASES, ids=lambda c: "%dx%d" % c)
PREC = pytest.mark.parametrize("f32", [False, True], ids=["fp16", "fp32"])


# --------------------------------------------------------------------------- #
# 1xx. per op
# --------------------------------------------------------------------------- #
@CANVAS
@PREC
def test_101_stem_conv1(nat, canvas_hw, f32):
    """the VALU stem: taps beyond the image are zero padding (not the canvas' NaN), outputs up to ceil(h/2) x ceil(w/2)"""
    g = _gen(101, f32)
    p = Prog(f32)
    t = p.b.stem(*_conv(g, 3, 64, 3, 2))
    p.head(nat, t, 8, 0, g)
    p.head(nat, t, 4, 1, g)
    _mixed_vs_alone(nat, p, canvas_hw, g, "stem conv1 %s" % ("fp32" if f32 else "fp16"))


def _prog_102(nat, f32):
    g = _gen(102, f32)
    p = Prog(f32)
    b = p.b
    t1 = b.stem(*_conv(g, 3, 64, 3, 2))
    t2 = b.conv(t1, *_conv(g, 64, 32, 3, 2), relu=True)                      # 1/4
    t3 = b.conv(t2, *_conv(g, 32, 32, 3, 1), relu=False)
    t4 = b.conv(t3, *_conv(g, 32, 32, 3, 1), relu=True, residual=t2)
    t5 = b.conv(t4, *_conv(g, 32, 48, 3, 2, bn=False), relu=False)          # 1/8, bias
    t6 = b.conv(t5, *_conv(g, 48, 48, 3, 1), relu=False, residual=t5)
    p.head(nat, t4, 8, 0, g)
    p.head(nat, t6, 8, 1, g)
    return p


@CANVAS
@PREC
def test_102_3x3_convs_stride_1_and_2_with_and_without_residual_and_relu(nat, canvas_hw, f32):
    """one-workgroup-per-tile kernel, both staging forms' masks, the residual prefetch, the NHWC store loop; a stride-2 conv
    writes up to the next level's extent (9 x 12 -> 5 x 6), whatever the canvas holds at that level"""
    for dma in (1, 0):                                                      # LDS-DMA staging and the register form
        nat.check(nat.lib().rtpe_set_option(b"tile_dma", dma))
        try:
            _mixed_vs_alone(nat, _prog_102(nat, f32), canvas_hw, _gen(1020, f32),
                            "3x3 convs %s tile_dma=%d" % ("fp32" if f32 else "fp16", dma))
        finally:
            nat.check(nat.lib().rtpe_set_option(b"tile_dma", 1))


@CANVAS
def test_103_fp16_conv_at_dilation_5_into_a_32_channel_slice(nat, canvas_hw):
    """the half body's in-place concat: dilations 5 and 2 into the two 32-channel slices of one tensor; at dilation 5 every
    tap but the centre one of a 9 x 12 map's border pixels lies beyond the image - in the canvas' other data, were it unmasked"""
    g = _gen(103)
    p = Prog(False)
    b = p.b
    t1 = b.stem(*_conv(g, 3, 64, 3, 2))
    t2 = b.conv(t1, *_conv(g, 64, 48, 3, 2), relu=True)
    cat = b.new_tensor(64, 2)
    b.conv(t2, *_conv(g, 48, 32, 3, 1, 5), relu=True, out=(cat, 32), cout_store=32)
    b.conv(t2, *_conv(g, 48, 32, 3, 1, 2), relu=True, out=(cat, 0), cout_store=32)
    p.head(nat, cat, 8, 0, g)
    p.head(nat, cat, 4, 1, g, k=3)
    _mixed_vs_alone(nat, p, canvas_hw, g, "fp16 dilated convs into slices")


@CANVAS
@PREC
def test_104_avgpool_down_to_the_2x1_map(nat, canvas_hw, f32):
    """AvgPool2d(3, 2, 1, count_include_pad=False) four times, 1/2 -> 1/32: the window and its divisor count the taps inside
    the image (a canvas tap would be NaN), the output extent is the image's.  The chain ends at 1/32, where the 64 x 32 image
    is 2 x 1 (pooled from 4 x 2) and the others 2 x 2: the extent table ends there, and a 32-pixel side has no pixel at
    1/64 - the existing entry refuses to pool the 64 x 32 image alone any further, so 2 x 1 -> 1 x 1 has nothing to be
    compared with"""
    g = _gen(104, f32)
    p = Prog(f32)
    t = p.b.stem(*_conv(g, 3, 64, 3, 2))
    levels = [t]
    for _ in range(4):
        levels.append(p.b.avgpool(levels[-1]))
    assert p.b.tensors[levels[-1]][1] == 5
    p.head(nat, levels[-1], 8, 0, g)
    p.head(nat, levels[2], 8, 1, g)
    alone = _mixed_vs_alone(nat, p, canvas_hw, g, "avgpool chain %s" % ("fp32" if f32 else "fp16"))
    assert alone[2][0].shape == (1, 8, 2, 1) and alone[0][0].shape == (1, 8, 2, 2)


@CANVAS
@PREC
def test_105_nearest_fuse_with_2x_and_4x_terms(nat, canvas_hw, f32):
    """hi + up(lo at 1/16) + up(mid at 1/8) with nearest_src on the image's own extents per term and axis: 3 x 3 and 5 x 6
    into 9 x 12, 3 x 3 and 6 x 5 into 12 x 9, 4 x 2 and 8 x 4 into 16 x 8 (the multiple-of-32 image: the rule is the shift, as
    in its forward alone, which runs fuse_rows_kernel).  Positive data and weights: every pixel of a source map holds its own
    number (checked on the 1/16 map, which the second output shows), so a wrong source index changes the sum"""
    g = _gen(105, f32)
    p = Prog(f32)
    b = p.b
    t1 = b.stem(*_conv(g, 3, 64, 3, 2, positive=True))
    hi = b.conv(t1, *_conv(g, 64, 16, 3, 2, positive=True))
    mid = b.conv(hi, *_conv(g, 16, 16, 3, 2, positive=True))
    lo = b.conv(mid, *_conv(g, 16, 16, 3, 2, positive=True))
    out = b.fuse([(hi, 0), (lo, 2), (mid, 1)], relu=False)
    p.head(nat, out, 8, 0, g)
    conv, _ = _conv(g, 16, 8, 1, bn=False, positive=True)
    b.conv(lo, conv, None, out_flag=nat.F_OUT_REFINED, nhwc=False)
    p.shapes[1] = (8, 4)
    alone = _mixed_vs_alone(nat, p, canvas_hw, g, "nearest fuse %s" % ("fp32" if f32 else "fp16"), positive=True)
    if f32:
        for a in alone:
            plane = a[1][0, 0].ravel()
            assert len(set(plane.tolist())) == plane.size, "two pixels of the 1/16 map hold the same number"


@CANVAS
@PREC
@pytest.mark.parametrize("data", ["int", "generic"])
def test_106_se_gate_sums_the_images_own_pixels_in_their_own_order(nat, canvas_hw, f32, data):
    """the gate, read through cam_combine.  ``int``: integer images, integer weights up to the SE input - the sum over the
    image's pixels is exact in any order, so equality with the image alone shows the masks and the divisor h * w alone;
    ``generic``: the fp32 sum depends on its order, so equality also shows the image's own row-major walk"""
    ints = data == "int"
    g = _gen(106, f32, ints)
    p = Prog(f32)
    b = p.b
    t1 = b.stem(*_conv(g, 3, 64, 3, 2, ints=ints))
    x2 = b.conv(t1, *_conv(g, 64, 16, 3, 2, ints=ints), relu=True)
    fc1, fc2 = nn.Linear(16, 8), nn.Linear(8, 16)
    with torch.no_grad():
        for fc in (fc1, fc2):
            fc.weight.copy_((torch.randn(fc.weight.shape, generator=g) / 4).half().float())
            fc.bias.copy_((torch.randn(fc.bias.shape, generator=g) / 4).half().float())
        if ints:
            fc1.weight.mul_(1.0 / 64)                   # the integer means are O(10): keep the sigmoid off its plateaus
    gate = b.se(x2, fc1, fc2)
    res = b.conv(x2, *_conv(g, 16, 16, 1))
    hdc = b.conv(x2, *_conv(g, 16, 16, 1))
    out = b.cam_combine(hdc, res, gate)
    p.head(nat, out, 8, 0, g)
    p.head(nat, out, 8, 1, g)
    _mixed_vs_alone(nat, p, canvas_hw, g, "se gate %s %s" % ("fp32" if f32 else "fp16", data), ints=ints)


@CANVAS
def test_107_fp32_nchw_head_at_canvas_widths_12_and_20(nat, canvas_hw):
    """the students' last op: conv 3x3 with bias, fp32, NCHW output only, 1 and 18 channels.  The canvas is 12 or 20 pixels
    wide at 1/4 (16-byte row pieces), the images 12, 9 and 8: the image with the odd width takes the element-wise stores
    inside the same launch; nothing is stored beyond an image, and the rest of the canvas is 0.0"""
    g = _gen(107)
    p = Prog(True)
    b = p.b
    t1 = b.stem(*_conv(g, 3, 64, 3, 2))
    t2 = b.conv(t1, *_conv(g, 64, 8, 3, 2), relu=True)
    assert nat.extent(canvas_hw[1], 2) in (12, 20)
    p.head(nat, t2, 1, 0, g, k=3)
    p.head(nat, t2, 18, 1, g, k=3)
    _mixed_vs_alone(nat, p, canvas_hw, g, "fp32 NCHW head")


# --------------------------------------------------------------------------- #
# 2xx. whole network
# --------------------------------------------------------------------------- #
_STUDENTS = {}


def _student100(golden_dir, body_half):
    if body_half not in _STUDENTS:
        from rtpe.students import AttentionStudent
        stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False, body_half=body_half).eval()
        stu.load_state_dict(S.student_sd(golden_dir, "s100"), strict=True)
        _STUDENTS[body_half] = stu.to(DEV)
    return _STUDENTS[body_half]


def _net_images():
    ims = []
    for (h, w), seed in zip(M.NET_SIZES, M.NET_SEEDS):
        n = 2 if (h, w) == (33, 47) else 1              # (the fixture's 33 x 47 case draws two images; image 0 is used)
        ims.append(synth.make_images(n, h, w, seed=seed)[0].to(DEV))
    return ims


def _canvas(ims, canvas_hw=None):
    from rtpe.students import pack_mixed
    canvas, sizes = pack_mixed(ims, canvas_hw)
    nan = torch.full_like(canvas, float("nan"))
    for n, (h, w) in enumerate(sizes):
        nan[n, :, :h, :w] = canvas[n, :, :h, :w]
    return nan, sizes


@pytest.fixture(scope="module")
def net_alone(nat, golden_dir):
    """``stu(x_n[None])`` for every image of the whole-network batch and both bodies: computed once"""
    out = {}
    ims = _net_images()
    for half in (False, True):
        stu = _student100(golden_dir, half)
        with torch.no_grad():
            out[half] = [tuple(t.clone() for t in stu(im[None])) for im in ims]
    return out


@pytest.mark.parametrize("body_half", [False, True], ids=["fp32_body", "half_body"])
def test_201_forward_mixed_gives_every_image_the_bits_of_its_own_forward(nat, golden_dir, net_alone, body_half):
    from rtpe.students import unpack_mixed
    stu = _student100(golden_dir, body_half)
    ims = _net_images()
    canvas, sizes = _canvas(ims)
    assert sizes == M.NET_SIZES and canvas.shape == (4, 3, 100, 140) and bool(torch.isnan(canvas).any())
    with torch.no_grad():
        att, det = stu.forward_mixed(canvas, sizes)
    assert att.shape == (4, 1, 25, 35) and det.shape == (4, 18, 25, 35) and att.dtype == det.dtype == torch.float32
    outside_a, outside_d = att.clone(), det.clone()
    for n, ((a, d), (wa, wd)) in enumerate(zip(unpack_mixed(att, det, sizes), net_alone[body_half])):
        assert torch.equal(a, wa[0]) and torch.equal(d, wd[0]), "image %d (%s)" % (n, sizes[n])
        outside_a[n, :, :a.shape[1], :a.shape[2]] = 0
        outside_d[n, :, :d.shape[1], :d.shape[2]] = 0
    assert bool((outside_a == 0).all()) and bool((outside_d == 0).all())              # (NaN == 0 is False)
    # the reference's CPU outputs for images 0 and 1 (fp32 body; the half body is within the same bound of it)
    g = np.load(os.path.join(golden_dir, "student_sizes.npz"))
    parts = unpack_mixed(att, det, sizes)
    for n, name in ((0, "33x47"), (1, "100x140")):
        wa, wd = S.fixture_case(g, "s100", name)
        S.within((parts[n][0][None].cpu().numpy(), parts[n][1][None].cpu().numpy()), (wa[:1], wd[:1]),
                 "forward_mixed image %d vs reference %s (%s)" % (n, name, "half body" if body_half else "fp32 body"))
    # the same images in reversed order, and in a canvas 32 larger on both sides: the same bits
    canvas_r, sizes_r = _canvas(ims[::-1])
    canvas_b, sizes_b = _canvas(ims, (132, 172))
    with torch.no_grad():
        att_r, det_r = stu.forward_mixed(canvas_r, sizes_r)
        att_b, det_b = stu.forward_mixed(canvas_b, sizes_b)
    assert att_b.shape == (4, 1, 33, 43)
    for n, (a, d) in enumerate(parts):
        ar, dr = unpack_mixed(att_r, det_r, sizes_r)[len(ims) - 1 - n]
        ab, db = unpack_mixed(att_b, det_b, sizes_b)[n]
        assert torch.equal(ar, a) and torch.equal(dr, d) and torch.equal(ab, a) and torch.equal(db, d), n
    assert bool((att_b[:, :, 25:] == 0).all()) and bool((det_b[:, :, :, 35:] == 0).all())


@pytest.mark.parametrize("body_half", [False, True], ids=["fp32_body", "half_body"])
def test_202_two_64x96_images_equal_the_tuned_fast_route(nat, golden_dir, body_half):
    """a mixed batch of equal multiple-of-32 images runs the general kernels, ``stu(x)`` of the pair the tuned fast ones:
    the same bits"""
    stu = _student100(golden_dir, body_half)
    x = synth.make_images(2, 64, 96, seed=141).to(DEV)
    with torch.no_grad():
        want = [t.clone() for t in stu(x)]
        att, det = stu.forward_mixed(x, [(64, 96), (64, 96)])
    assert torch.equal(att, want[0]) and torch.equal(det, want[1]) and float(det.abs().max()) > 0


def test_203_a_plain_320x320_forward_after_a_mixed_one_keeps_its_bits(nat, golden_dir):
    """as test 205 of tests/test_student_sizes_gpu.py for ragged shapes: neither the workspace cache nor the tuner carries
    anything over from a mixed batch - which is never tuned, whatever its canvas size"""
    from rtpe.students import AttentionStudent, pack_mixed
    x = synth.make_images(1, 320, 320, seed=99).to(DEV)

    def fresh():
        stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False).eval()
        stu.load_state_dict(S.student_sd(golden_dir, "s100"), strict=True)
        return stu.to(DEV)
    with torch.no_grad():
        want = [t.clone() for t in fresh()(x)]
    stu = fresh()
    canvas, sizes = pack_mixed([synth.make_images(1, 64, 96, seed=3)[0].to(DEV), synth.make_images(1, 96, 64, seed=4)[0].to(DEV)])
    assert canvas.shape == (2, 3, 96, 96)
    with torch.no_grad():
        stu.forward_mixed(canvas, sizes)
        eng = stu._engine(x.device)
        assert not eng._tuned                                   # a canvas of multiples of 32 is not tuned either
        n_ints = ctypes.c_int32()
        nat.check(nat.lib().rtpe_hrnet_tuned_ints(eng._h, ctypes.byref(n_ints)))
        buf = (ctypes.c_int32 * n_ints.value)()
        assert nat.lib().rtpe_hrnet_export_tuned(eng._h, 2, 96, 96, buf, n_ints.value) != 0
        got = stu(x)
        stu.forward_mixed(canvas, sizes)
        again = stu(x)
    for a, b_, c in zip(got, want, again):
        assert torch.equal(a, b_) and torch.equal(c, b_)


# --------------------------------------------------------------------------- #
# 3xx. StudentPipeline.call_mixed
# --------------------------------------------------------------------------- #
class _BlobMixed(torch.nn.Module):
    """runs the real student (so that both forwards take the sizes) and hands out prepared blob-bearing det maps instead of
    its own: seeded networks find no people.  ``forward_mixed`` lays the maps of the images into the det canvas; whatever
    the student left outside the regions stays"""

    def __init__(self, stu, dets):
        super().__init__()
        self.stu, self.dets = stu, dets          # {(h, w): det (1, J + 1, ceil(h/4), ceil(w/4))}

    def forward(self, x, out_hw=None, alt=None):
        att, det = self.stu(x)
        want = self.dets[tuple(x.shape[2:])]
        assert x.shape[0] == 1 and det.shape == want.shape
        return att, want.clone()

    def forward_mixed(self, canvas, sizes):
        att, det = self.stu.forward_mixed(canvas, sizes)
        det = det.clone()
        for n, hw in enumerate(sizes):
            d = self.dets[tuple(hw)]
            det[n, :, :d.shape[2], :d.shape[3]] = d[0]
        return att, det


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_301_call_mixed_equals_the_pipeline_on_every_image_alone(nat, golden_dir, match_on):
    from rtpe.engine import StudentPipeline
    sizes = [(100, 140), (64, 96), (96, 128)]
    dets = {hw: _det((-(-hw[0] // 4), -(-hw[1] // 4)), (51 + i,)).to(DEV) for i, hw in enumerate(sizes)}
    ims = [synth.make_images(1, h, w, seed=70 + i)[0].to(DEV) for i, (h, w) in enumerate(sizes)]
    pipe = StudentPipeline(_BlobMixed(_student100(golden_dir, False), dets), _parser(match_on), DEV)
    got = pipe.call_mixed(ims)
    assert len(got) == 3
    for n, im in enumerate(ims):
        want = pipe(im[None])
        assert len(want) == 1 and _n_people(want[0][0]) >= 1, "an empty decode shows nothing"
        _same_people(got[n], want[0])
    # mixed batches are not streamed, and a tensor batch keeps its one decode size
    with pytest.raises(ValueError, match="call_mixed"):
        next(pipe.stream(iter([ims])))
    with pytest.raises(ValueError, match="one decode size"):
        pipe(ims[0][None], out_hw=[(100, 140)])
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- #
# 4xx. refusals of the C side, before the first launch
# --------------------------------------------------------------------------- #
def test_401_c_side_refusals(nat, golden_dir):
    from rtpe.students import AttentionStudentSteps
    from rtpe.third_party.pose_higher_hrnet import Engine, PoseHigherResolutionNet
    L = nat.lib()
    g = _gen(401)
    p = Prog(False)
    t = p.b.stem(*_conv(g, 3, 64, 3, 2))
    p.head(nat, t, 8, 0, g)
    p.head(nat, t, 4, 1, g)
    eng = _engine(p)
    canvas = _nan_canvas(_images(M.OP_SIZES, g), (64, 47))
    for sizes, msg in (([(31, 47), (47, 33), (64, 32)], "at least 32"), ([(33, 47), (47, 33), (65, 32)], "larger than"),
                       ([(33, 48), (47, 33), (64, 32)], "larger than")):
        assert _forward_mixed_raw(nat, eng, p.shapes, canvas, sizes, expect_error=True) == -1
        assert msg in L.rtpe_last_error_string().decode(), (sizes, L.rtpe_last_error_string())
    # a teacher handle (no any_size property) and a Steps program (a second input), at a canvas both would take plainly
    teacher = Engine(PoseHigherResolutionNet().eval().compile_program(), 0)
    x = torch.zeros(2, 3, 64, 64)
    assert _forward_mixed_raw(nat, teacher, [(34, 2), (17, 1)], x, [(64, 64), (32, 64)], expect_error=True) == -1
    assert "any_size" in L.rtpe_last_error_string().decode()
    steps = Engine(AttentionStudentSteps(None, "cpu", 48, 17, 1, True, None, False).eval().compile_program(("att_divisor", None)), 0)
    assert _forward_mixed_raw(nat, steps, [(1, 2), (18, 2)], x, [(64, 64), (32, 64)], expect_error=True) == -1
    assert "second input" in L.rtpe_last_error_string().decode()
    # and the accepted call after all of them
    _forward_mixed_raw(nat, eng, p.shapes, canvas, M.OP_SIZES)
