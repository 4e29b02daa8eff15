"""CPU tests of ``AttentionStudentStepsHalf``: the class and its refusals, the compiled program, the rounding points of the three
fp16 ops it adds (aux pack, resize, gate_mul), the faults their data can see, and the fixture.

The rounding points are pinned HERE, in the style of tests/test_student_half_host.py: each reference is float64 arithmetic with
an explicit round to fp32 and then to fp16 (``R``) wherever PyTorch-CPU's half op rounds, asserted bit for bit against the op
itself with oneDNN on and off:

  alt.half()        round to nearest even per element; beyond the fp16 range: infinity
  F.interpolate     (bilinear, align_corners=False) fp32 arithmetic on the fp16 values - the fp32 op's fma(scale, o + 0.5, -0.5)
                    coordinate, clamps and weights; the taps combined in PyTorch's order (ly * lx first, then v01 * w01 and three
                    fmas), NOT with the fp32 op's three fmas, which differ in the last fp32 bit at scales that are no fp32
                    numbers - and ONE rounding of the result
  torch.cat         exact
  att / divisor     the fp32 quotient, one rounding
  sigmoid           the fp32 sigmoid, one rounding (the emitted ``att`` is that value)
  stem_out * att    one rounding per element

The case tables and data of tests/test_steps_half_gpu.py live here."""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_conv_exact_host as C
import test_student_half_host as H
import test_student_ops_host as T
from oracle import student_ops as so
from test_student_half_host import R, F32, is_f16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
D = torch.float64
SEED = 8123
PAD = 5                                                # zero channels behind (r, g, b) in a packed row of 8 halves

# the fixture's cases (tools/gen_golden_steps_half.py): name, inplanes, seed of the weights, N, H, W, seeds of x and alt, divisor
STEPS_HALF_CASES = (("p48_33x47_nodiv", 48, 4, 2, 33, 47, 121, 122, None), ("p48_33x47_div20", 48, 4, 2, 33, 47, 121, 122, 20.0),
                    ("p48_64x96_nodiv", 48, 4, 2, 64, 96, 123, 124, None), ("p48_64x96_div20", 48, 4, 2, 64, 96, 123, 124, 20.0),
                    ("p80_64x64_div20", 80, 5, 1, 64, 64, 125, 126, 20.0))
SHAPES_FILE = {48: "student_steps_shapes.json", 80: "student_steps80_shapes.json"}
MUTATIONS = {"pack": ("no_round", "pad_nonzero", "swap_rb"), "resize": ("no_round", "double_round", "fp32_op_fmas"),
             "gate": ("no_round_quotient", "no_round_product")}


def _g(*key):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _mut(op, mutate):
    assert mutate is None or mutate in MUTATIONS[op], (op, mutate)
    return mutate


# --------------------------------------------------------------------------- #
# references
# --------------------------------------------------------------------------- #
def pack16(aux, mutate=None):
    """(N, 3, H, W) fp32 values -> the packed row of 8: r, g, b rounded to fp16, five zeros"""
    m = _mut("pack", mutate)
    assert so.is_f32(aux)
    a = aux[:, [2, 1, 0]] if m == "swap_rb" else aux
    a = a if m == "no_round" else a.half().double()
    pad = torch.full((aux.shape[0], PAD) + tuple(aux.shape[2:]), 1.0 if m == "pad_nonzero" else 0.0, dtype=D)
    return torch.cat([a, pad], 1)


def resize16(x, Ho, Wo, mutate=None):
    """F.interpolate(x.half(), (Ho, Wo), mode="bilinear"): the coordinates, clamps and weights of oracle/student_ops.py
    ``resize`` (the fp32 op's), the four taps combined as PyTorch-CPU's kernel combines them - the weights multiplied first
    (ly * lx, rounded to fp32), then v01 * w01, fma(v00, w00, .), fma(v10, w10, .), fma(v11, w11, .) - and ONE rounding of the
    fp32 result to fp16.
      ``no_round``       the fp32 result kept
      ``double_round``   the sum of the upper row's two terms rounded to fp16 before the lower row's are added
      ``fp32_op_fmas``   the three fmas of the fp32 op (fma(v0, l0, v1 * l1) along x, the same along y): the same value but for
                         the last fp32 bit at scales that are no fp32 numbers - next to a tie a whole fp16 step"""
    m = _mut("resize", mutate)
    assert is_f16(x)
    r = so.resize(x, Ho, Wo)
    if m == "fp32_op_fmas":
        return R(r.out)
    ay, ax = r.y, r.x
    rows0, rows1 = x[:, :, ay.i0], x[:, :, ay.i1]
    v00, v01, v10, v11 = rows0[..., ax.i0], rows0[..., ax.i1], rows1[..., ax.i0], rows1[..., ax.i1]
    w = lambda ly, lx: F32(ly.view(-1, 1) * lx.view(1, -1))              # (Ho, Wo)
    acc = F32(v00 * w(ay.l0, ax.l0) + F32(v01 * w(ay.l0, ax.l1)))         # (a float64 product of two fp32 numbers is exact: one fma)
    if m == "double_round":
        acc = R(acc)
    acc = F32(v10 * w(ay.l1, ax.l0) + acc)
    acc = F32(v11 * w(ay.l1, ax.l1) + acc)
    return acc if m == "no_round" else R(acc)


def gate_arg(logits, div, mutate=None):
    """the sigmoid's argument: the fp16 logit, or its fp32 quotient by ``div`` rounded once"""
    m = _mut("gate", mutate)
    assert is_f16(logits)
    if not div:
        return logits
    q = F32(logits / float(div))
    return q if m == "no_round_quotient" else R(q)


def gate16(x, att, mutate=None):
    """x * att (att (N, 1, H, W) fp16 values, broadcast over the channels): one rounding per element"""
    m = _mut("gate", mutate)
    assert is_f16(x) and is_f16(att)
    return F32(x * att) if m == "no_round_product" else R(x * att)


# --------------------------------------------------------------------------- #
# data of the op tests (CPU here, the same arrays on the GPU)
# --------------------------------------------------------------------------- #
PACK_CASES = [(1, 32, 32), (3, 96, 64)]
# (source ds, target ds) as tests/test_student_ops_host.py RESIZE_RATIOS: ratios 4, 2, 8, 1 and the upscales 1/2 and 1/4
RESIZE_CASES = [(s, t, N, H, W, order) for (s, t) in T.RESIZE_RATIOS for (N, H, W, order) in ((1, 32, 96, "before"), (3, 32, 96, "after"))]
RESIZE_RAGGED = (2, 33, 47)                            # 33 x 47 -> 9 x 12: scales 3.667 and 3.917, no fp32 numbers
RESIZE_P = 8
GATE_CASES = [(P, div, order) for P, div in ((8, None), (8, 20.0), (8, 7.5), (48, 7.5)) for order in ("before", "after")]
GATE_SHAPE = (3, 32, 32)
CONV5_FIRST = [(2, 32, 32), (2, 33, 47)]               # 8 -> 56 (3 and 50 logical) at full resolution
CONV5_SECOND = [(2, 32, 32), (2, 33, 47)]              # 56 -> 48 at 1/2: maps 16 x 16 and 17 x 24, into [56, 104) of 104


@functools.lru_cache(maxsize=4)
def pack_data(N, H, W, gpu=False):
    """fp32 values with more than 11 significant bits (multiples of 2^-13 up to 4), exact ties in [1, 2) and [2, 4) (odd
    multiples of 2^-11 and 2^-10: half an fp16 step, both parities of the kept bit), zeros of both signs, values below the
    smallest fp16 normal.  On the CPU also values beyond the fp16 range (the GPU test reads the row back through a selection
    conv, which cannot carry an infinity)."""
    g = _g(1, N, H, W)
    aux = torch.randint(-2 ** 15, 2 ** 15, (N, 3, H, W), generator=g).double() * 2.0 ** -13
    ties = (1024 + torch.arange(0, 64, dtype=D)) * 2.0 ** -10 + 2.0 ** -11           # halfway between two halves of [1, 2)
    aux[0, 0, 0, :32] = ties[:32]
    aux[0, 1, 1, :32] = -2 * ties[32:]
    aux[0, 2, 2, :4] = torch.tensor([0.0, -0.0, 2.0 ** -15 + 2.0 ** -26, -2.0 ** -24 * 1.5], dtype=D)
    if not gpu:
        aux[0, 2, 3, :4] = torch.tensor([65520.0, -1e30, 65519.0, 70000.0]).double()
    assert so.is_f32(aux)
    return types.SimpleNamespace(aux=aux, want=pack16(aux))


def _phys8(v):
    """(N, 3, H, W) -> the physical row of 8: the three channels and five zeros"""
    return torch.cat([v, torch.zeros((v.shape[0], PAD) + tuple(v.shape[2:]), dtype=D)], 1)


@functools.lru_cache(maxsize=4)
def resize_data(src_ds, tgt_ds, N, Hh, W):
    """tests/test_student_ops_host.py ``resize_data`` in rows of 8 halves: the source is the packed second input or a
    sub-sampled copy of it (integers of +-2047, all 11 bits of a half: an average of two or four of them and a product with
    a weight of 1/4 or 1/8 need more, so every rounding of every ratio but 1 acts), the target's first RESIZE_P channels a 1x1
    integer mix of the map at the target's resolution"""
    g = _g(2, src_ds, tgt_ds, N, Hh, W)
    top = max(src_ds, tgt_ds)
    base = H._ints(g, -2047, 2047, (N, 3, Hh >> top, W >> top))
    aux, chain = T.aux_feed(base, top, g)
    if src_ds == 0 and top > 0:          # a downscale reads the pixels between those the sub-sampling keeps: 11 bits there too
        aux = H._ints(g, -2047, 2047, tuple(aux.shape))
        aux[:, :, ::1 << top, ::1 << top] = base
        chain[0] = so.aux_pack(aux)
    d = types.SimpleNamespace(aux=aux, chain=chain, top=top)
    r = types.SimpleNamespace(N=N, H=Hh, W=W, aux=d.aux, top=d.top)
    r.src = _phys8(d.chain[src_ds][:, :3])
    w = torch.zeros(RESIZE_P, 8, 1, 1, dtype=D)
    w[:, :2] = torch.eye(2, dtype=D).repeat(RESIZE_P // 2, 1).view(RESIZE_P, 2, 1, 1)       # (one channel each: the sums stay halves)
    r.l_n = T.make_layer(w, torch.ones(RESIZE_P, dtype=D), torch.zeros(RESIZE_P, dtype=D), 1)
    r.neigh = H.apply1x1(_phys8(d.chain[tgt_ds][:, :3]), r.l_n)
    r.out = resize16(r.src, Hh >> tgt_ds, W >> tgt_ds)
    r.want = torch.cat([r.neigh, r.out], 1)
    return r


@functools.lru_cache(maxsize=2)
def resize_ragged_data():
    """the second input at 33 x 47 (multiples of 1/8 up to +-100, a LAB image's span) to the map at 1/4, 9 x 12"""
    N, Hh, W = RESIZE_RAGGED
    g = _g(3)
    aux = H._ints(g, -800, 800, (N, 3, Hh, W)) / 8
    r = types.SimpleNamespace(N=N, H=Hh, W=W, aux=aux, src=_phys8(aux))
    r.out = resize16(r.src, 9, 12)
    return r


@functools.lru_cache(maxsize=1)
def resize_lab_data():
    """the fixture's own second input at 2 x 33 x 47 (a seeded LAB image: arbitrary fp32 values) to 9 x 12: the data on which
    the fp32 op's three fmas give another half than PyTorch (``fp32_op_fmas``)"""
    aux = steps_alt(2, 33, 47, 122).double()
    r = types.SimpleNamespace(N=2, H=33, W=47, aux=aux, src=_phys8(aux.half().double()))
    r.out = resize16(r.src, 9, 12)
    return r


def sub_layer():
    """the fp16 k3 s2 conv that keeps the pixels at even positions of channels 0..2 of a row of 8"""
    return T.make_layer(T.sub_weights(8), torch.ones(8, dtype=D), torch.zeros(8, dtype=D), 2)


def gate_logits(div, count, seed):
    """``count`` fp16 logits (multiples of 1/8): the points at which the fp16 sigmoid of l / div is 0.5, 1 and 0, their
    neighbours, and random values of |l / div| <= 12"""
    d = float(div) if div else 1.0
    fixed = [0.0, 0.125, -0.125, 9 * d, 20 * d, 100 * d, -18 * d, -30 * d, -104 * d, 12 * d, -12 * d]
    fixed = [float(torch.tensor(v).half()) for v in fixed]
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(int(-12 * d * 8), int(12 * d * 8) + 1, (count - len(fixed),), generator=g).double() / 8
    l = torch.cat([torch.tensor(fixed, dtype=D), rnd])
    assert is_f16(l)
    return l[torch.randperm(count, generator=g)]


@functools.lru_cache(maxsize=4)
def gate_data(P, div):
    """the second input carries the logits in its first plane and small integers in the other two (tests/
    test_student_ops_host.py ``sig_data``): the logits reach the op through a 1x1 selection into a row of 8, the gated tensor
    (P + 8 channels, integers up to +-22: a product with an 11-bit sigmoid needs 16 bits) through a 1x1 integer mix, the
    neighbour's P channels through another"""
    N, Hh, W = GATE_SHAPE
    g = _g(4, P, int((div or 0) * 2))
    l = gate_logits(div, N * Hh * W, SEED + P + int((div or 0) * 2)).view(N, 1, Hh, W)
    aux = torch.cat([l, H._ints(g, -9, 9, (N, 2, Hh, W))], 1)
    r = types.SimpleNamespace(N=N, H=Hh, W=W, aux=aux, logits=l, packed=pack16(aux), arg=gate_arg(l, div))
    w_l = torch.zeros(8, 8, 1, 1, dtype=D)
    w_l[0, 0] = 1
    r.l_logit = T.make_layer(w_l, torch.ones(8, dtype=D), torch.zeros(8, dtype=D), 1)
    w_x = torch.zeros(P + 8, 8, 1, 1, dtype=D)
    w_x[:, 1:3] = H._ints(g, -1, 1, (P + 8, 2, 1, 1))
    r.l_x = T.make_layer(w_x, torch.ones(P + 8, dtype=D), H._ints(g, -4, 4, (P + 8,)), 1)
    w_n = torch.zeros(P, 8, 1, 1, dtype=D)
    w_n[:, 1:3] = H._ints(g, -1, 1, (P, 2, 1, 1))
    r.l_n = T.make_layer(w_n, torch.ones(P, dtype=D), H._ints(g, -4, 4, (P,)), 1)
    r.x, r.neigh = H.apply1x1(r.packed, r.l_x), H.apply1x1(r.packed, r.l_n)
    return r


@functools.lru_cache(maxsize=4)
def conv5_data(N, Hh, W):
    """the two 5x5 stride-2 layers of ``alt_img_stem`` on order-independent data (tests/test_conv_exact_host.py ``_layer``):
    3 -> 50 + BN + ReLU on the packed second input (integers of +-3), then 50 -> 48 + BN + ReLU on its output (multiples of
    1/2).  ``u`` is the first layer's physical output (56 channels, 50 used), ``v`` the second's"""
    g = _g(5, N, Hh, W)
    aux = H._ints(g, -3, 3, (N, 3, Hh, W))
    r = types.SimpleNamespace(N=N, H=Hh, W=W, aux=aux)
    r.l1 = C._layer(3, 50, 5, 2, g)
    r.l2 = C._layer(50, 48, 5, 2, g, density=0.3)
    u = C._ref_layer(aux, r.l1, 5, 2, True, True, quantum=1.0)
    r.u = torch.cat([u, torch.zeros((N, 6) + tuple(u.shape[2:]), dtype=D)], 1)
    r.v = C._ref_layer(u, r.l2, 5, 2, True, True, quantum=0.5)
    assert is_f16(r.u) and is_f16(r.v) and (r.u > 0).double().mean() > 0.2 and (r.v > 0).double().mean() > 0.2
    return r


# --------------------------------------------------------------------------- #
# (1) the references are PyTorch-CPU's half ops
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", PACK_CASES, ids=str)
def test_pack_reference_is_alt_half_and_a_cat(case):
    d = pack_data(*case)

    def check():
        h = d.aux.float().half()
        assert torch.equal(torch.cat([h, torch.zeros((h.shape[0], PAD) + tuple(h.shape[2:]), dtype=torch.float16)], 1).double(), d.want)
    H._both_backends(check)
    a = d.aux.float()
    assert torch.isinf(d.want).sum() == 3 and float(d.want[0, 2, 3, 2]) == 65504.0           # 65520, -1e30, 70000; 65519 stays
    assert not torch.equal(a.half().double()[:, :, :4], d.aux[:, :, :4])                       # rows 0..3: ties, a denormal
    assert float(d.want[0, 0, 0, 0]) == 1.0 and float(d.want[0, 0, 0, 1]) == 1.0 + 2.0 ** -9  # ties go to the even neighbour
    for m in MUTATIONS["pack"]:
        assert not torch.equal(pack16(d.aux, m)[:, :, :3], d.want[:, :, :3]), m


@pytest.mark.parametrize("case", RESIZE_CASES[::2], ids=str)
def test_resize_reference_is_pytorchs_half_interpolate(case):
    s, t, N, Hh, W, _ = case
    d = resize_data(s, t, N, Hh, W)

    def check():
        y = F.interpolate(d.src.half(), (Hh >> t, W >> t), mode="bilinear", align_corners=False)
        assert torch.equal(y.double(), d.out)
        y = F.interpolate(d.src[:, :3].half().contiguous(memory_format=torch.channels_last), (Hh >> t, W >> t), mode="bilinear")
        assert torch.equal(y.double(), d.out[:, :3])
    H._both_backends(check)
    assert not d.out[:, 3:].any()                                       # the pad channels: interpolated zeros
    for m in ("no_round", "double_round"):
        assert torch.equal(resize16(d.src, Hh >> t, W >> t, m), d.out) == (s == t), (m, case)      # (ratio 1: a copy)


def test_ragged_resize_reference_is_pytorchs_half_interpolate():
    d = resize_ragged_data()

    def check():
        y = F.interpolate(d.src.half(), (9, 12), mode="bilinear", align_corners=False)
        assert torch.equal(y.double(), d.out)
    H._both_backends(check)
    for m in ("no_round", "double_round"):
        assert not torch.equal(resize16(d.src, 9, 12, m), d.out), m
    assert not d.out[:, 3:].any()


def steps_alt(n, h, w, seed):
    """the alt image of a fixture case: a seeded RGB image in LAB (tools/gen_golden_steps_half.py)"""
    from oracle import student_ref
    rgb = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))
    lab = student_ref.rgb2lab(rgb.permute(0, 2, 3, 1).numpy()).astype(np.float32)
    return torch.from_numpy(lab).permute(0, 3, 1, 2).contiguous()


def test_resize_reference_on_a_lab_image_and_the_fp32_ops_fmas_are_seen():
    """the fixture's own second input (2 x 33 x 47, arbitrary fp32 values rounded to fp16) to 9 x 12: PyTorch's half op bit
    for bit, and the three fmas of the fp32 op give another half in one element of 648 (L of image 1 at (2, 1): 53.9375
    against 53.96875, the fp32 values on either side of the tie 53.953125) - the fault that moved the attention map of image 1
    by six elements on the GPU before the fp16 form took PyTorch's order"""
    x = _phys8(steps_alt(2, 33, 47, 122).half().double())
    want = resize16(x, 9, 12)

    def check():
        y = F.interpolate(x.half(), (9, 12), mode="bilinear", align_corners=False)
        assert torch.equal(y.double(), want)
    H._both_backends(check)
    other = resize16(x, 9, 12, "fp32_op_fmas")
    assert int((other != want).sum()) == 1 and float(want[1, 0, 2, 1]) == 53.96875 and float(other[1, 0, 2, 1]) == 53.9375


@pytest.mark.parametrize("P,div", sorted(set(c[:2] for c in GATE_CASES), key=str), ids=str)
def test_gate_mul_reference_is_pytorchs_half_ops(P, div):
    d = gate_data(P, div)

    def check():
        q = d.logits.half() / div if div else d.logits.half()
        assert torch.equal(q.double(), d.arg)
        att = torch.sigmoid(q)
        ok, near, took = H.sigmoid16_check(att.double(), d.arg)
        assert ok and near <= 0.004, (near, took)       # (2 (4 + 12) / 2^13: test_sigmoid_budget_in_fp16)
        y = d.x.half() * att.expand(d.x.shape)
        assert torch.equal(y.double(), gate16(d.x, att.double()))
    H._both_backends(check)
    att = H.sigmoid16(d.arg)
    # the exact points: 0.5 at 0, 1 from 9 up, 0 from -18 down - the float64 sigmoid there is further from an fp16 rounding
    # boundary than any fp32 sigmoid within its budget can reach
    a = d.arg
    for sel, v in ((a == 0, 0.5), (a >= 9, 1.0), (a <= -18, 0.0)):
        assert sel.any() and bool((att[sel] == v).all())
    if div:
        assert not torch.equal(gate_arg(d.logits, div, "no_round_quotient"), d.arg)
    assert not torch.equal(gate16(d.x, att, "no_round_product"), gate16(d.x, att))


def test_sigmoid_budget_in_fp16():
    """how the 4 + |a| fp32-ulp budget of the fp32 sigmoid carries to fp16: the kernel rounds an fp32 value within the budget
    of the true sigmoid once, so it gives the correctly rounded half of the true value unless the true value lies within the
    budget of a boundary between two halves; there it may give either neighbour, nowhere anything else.  One fp16 step is 2^13
    fp32 ulps, so about 2 (4 + |a|) / 2^13 of arbitrary arguments are that close: 0.1 to 0.4 % on |a| <= 12"""
    arg = gate_arg(gate_logits(7.5, 100000, 5), 7.5)
    ok, near, took = H.sigmoid16_check(H.sigmoid16(arg), arg)
    assert ok and took == 0 and 0.001 < near <= 0.004, near


@pytest.mark.parametrize("shape", CONV5_FIRST, ids=str)
def test_conv5_data_is_exact_in_any_order_and_matches_pytorchs_half_convs(shape):
    d = conv5_data(*shape)
    conv1, bn1, conv2, bn2 = d.l1[0], d.l1[1], d.l2[0], d.l2[1]

    def check():
        with torch.no_grad():
            u = torch.relu(bn1.eval()(conv1(d.aux.half()).float()).half())
            assert torch.equal(u.double(), d.u[:, :50])
            v = torch.relu(bn2.eval()(conv2(u).float()).half())
            assert torch.equal(v.double(), d.v)
    H._both_backends(check)
    assert tuple(d.u.shape[2:]) == (-(-shape[1] // 2), -(-shape[2] // 2)) and tuple(d.v.shape[2:]) == (-(-shape[1] // 4), -(-shape[2] // 4))


# --------------------------------------------------------------------------- #
# (2) the class, its refusals, its program
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=2)
def half_steps(P=48):
    from rtpe.students import AttentionStudentStepsHalf
    return AttentionStudentStepsHalf(None, "cpu", P, 17, 1, True, None, False)


def steps_sd(P, seed):
    from oracle import synth
    shapes = json.load(open(os.path.join(GOLDEN, SHAPES_FILE[P])))["shapes"]
    return synth.make_state_dict({k: tuple(v) for k, v in shapes.items()}, seed, "W1")


@pytest.mark.parametrize("P", (48, 80))
def test_the_class_constructs_without_a_gpu_and_stores_what_the_contract_says(P):
    """fp16 parameters, fp32 BatchNorm (int64 counters) in stem and body: the dtypes of the reference module after
    BN_convert_float(model.half()); an fp32 checkpoint loads into it and the BatchNorms keep its fp32 values"""
    from rtpe.students import AttentionStudentSteps
    m = half_steps(P)
    assert isinstance(m, AttentionStudentSteps)
    sd = m.state_dict()
    shapes = json.load(open(os.path.join(GOLDEN, SHAPES_FILE[P])))["shapes"]
    assert {k: list(v.shape) for k, v in sd.items()} == shapes and len(sd) == 340
    bn = {n for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)}
    for k, v in sd.items():
        owner = k.rsplit(".", 1)[0]
        want = (torch.int64 if k.endswith("num_batches_tracked") else torch.float32) if owner in bn else torch.float16
        assert v.dtype == want, (k, v.dtype, want)
    ck = steps_sd(P, 4)
    assert all(v.dtype != torch.float16 for v in ck.values())
    m.load_state_dict(ck, strict=True)
    for k in ("alt_img_stem.0.weight", "steps.0.se.fc.0.weight", "att_top.0.bias", "steps.3.weight"):
        assert m.state_dict()[k].dtype == torch.float16 and torch.equal(m.state_dict()[k], ck[k].half()), k
    for k in ("alt_img_stem.1.running_var", "steps.1.hdc_top.1.weight", "mid_stem.1.bias"):
        assert m.state_dict()[k].dtype == torch.float32 and torch.equal(m.state_dict()[k], ck[k]), k


def test_the_refusals():
    from rtpe.students import AttentionStudentSteps, AttentionStudentStepsHalf
    with pytest.raises(ValueError, match="half_precision=True"):
        AttentionStudentStepsHalf(None, "cpu", 48, 17, 1, False)
    for P in (100, 50, 4, 0):
        with pytest.raises(ValueError, match="multiple of 8"):
            AttentionStudentStepsHalf(None, "cpu", P)
    with pytest.raises(TypeError):
        AttentionStudentStepsHalf(None, "cpu", 48, body_half=True)
    with pytest.raises(NotImplementedError, match="no half body"):             # the public keyword of the fp32 class: as it was
        AttentionStudentSteps(None, "cpu", 48, body_half=True)
    assert AttentionStudentSteps._HALF_BODY is False


def test_mixed_batches_are_refused_before_any_gpu_work():
    """``forward_mixed`` and the pipeline's two mixed entries: NotImplementedError that names the missing masked fp16 forms,
    with CPU tensors (nothing is packed, nothing launched: a CPU tensor would fail ``require_gpu`` first otherwise)"""
    from rtpe.engine import StudentPipeline
    m = half_steps().eval()
    ims = [torch.zeros(3, 33, 47), torch.zeros(3, 64, 40)]
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        m.forward_mixed(torch.zeros(2, 3, 64, 47), [(33, 47), (64, 40)], alt=torch.zeros(2, 3, 64, 47))
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        m.forward_mixed(None, None)
    pipe = StudentPipeline.__new__(StudentPipeline)                  # (the constructor makes streams: no GPU here)
    pipe.model = m
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        pipe.call_mixed(ims, alt=ims)
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        pipe._mixed_begin((ims, ims))                                # what stream_mixed does with every batch first


def test_the_fp32_class_compiles_the_program_it_always_did():
    """tests/golden/steps_program_default.json: the op list, the gate_mul divisor bits and the tensors of
    ``AttentionStudentSteps`` at inplanes 48 and 80, with and without a divisor, recorded before the half class existed"""
    from rtpe.students import AttentionStudentSteps
    want = json.load(open(os.path.join(GOLDEN, "steps_program_default.json")))
    assert sorted(want) == ["steps48_div20", "steps48_nodiv", "steps80_div20", "steps80_nodiv"]
    for P in (48, 80):
        m = AttentionStudentSteps(None, "cpu", P, 17, 1, True, None, False)
        for div in (None, 20.0):
            p = m.compile_program(("att_divisor", div))
            w = want["steps%d_%s" % (P, "nodiv" if div is None else "div20")]
            assert H.program_rows(p) == w["rows"], (P, div)
            assert [int(d.reserved[0]) for d, n in zip(p.ops, p.names) if n.startswith("gate_mul")] == w["divisor_bits"]
            assert [[int(t.channels), int(t.ds_log2), int(t.reserved)] for t in p.tensors] == w["tensors"]


@pytest.mark.parametrize("P", (48, 80))
def test_the_half_program_has_no_cast_no_fp32_op_and_rows_of_eight(P):
    from rtpe import _native as nat
    m = half_steps(P)
    m.load_state_dict(steps_sd(P, 4), strict=True)
    p = m.compile_program(("att_divisor", 20.0))
    kinds = [d.kind for d in p.ops]
    assert nat.OP_CAST not in kinds and p.any_size and p.has_aux
    assert kinds.count(nat.OP_AUX_PACK) == 1 and kinds.count(nat.OP_RESIZE) == 1 and kinds.count(nat.OP_GATE_MUL) == 1
    assert kinds.count(nat.OP_SE) == 6 and kinds.count(nat.OP_CAM_COMBINE) == 6 and kinds.count(nat.OP_AVGPOOL) == 2
    assert not any(d.flags & nat.F_F32 for d in p.ops)
    assert all(t.channels % 8 == 0 and t.reserved == 2 for t in p.tensors)
    assert all(d.out_coff % 8 == 0 and d.in_coff % 8 == 0 and d.res_coff % 8 == 0 for d in p.ops)
    op = lambda k: [d for d in p.ops if d.kind == k][0]
    ch = lambda t: p.tensors[t].channels
    pack, rs, gm = op(nat.OP_AUX_PACK), op(nat.OP_RESIZE), op(nat.OP_GATE_MUL)
    assert ch(pack.out_t) == 8 and p.tensors[pack.out_t].ds_log2 == 0
    # cat1 = [mid stem P | alt 3 | 0 x 5], cat2 = [gated P + 3 | 0 x 5 | alt stem P]
    assert rs.in_t == pack.out_t and ch(rs.out_t) == P + 8 and (rs.out_coff, rs.cout) == (P, 8)
    cat1, cat2 = rs.out_t, gm.out_t
    assert gm.res_t == cat1 and ch(cat2) == 2 * P + 8 and (gm.out_coff, gm.cout) == (0, P + 8) and gm.flags & nat.F_OUT_PREDS
    assert np.frombuffer(np.int32(gm.reserved[0]).tobytes(), np.float32)[0] == 20.0
    into1 = [d for d in p.ops if d.kind == nat.OP_CONV and d.out_t == cat1]
    assert len(into1) == 1 and (into1[0].out_coff, into1[0].reserved[2], into1[0].cout) == (0, P, P)
    k5 = [d for d in p.ops if d.kind == nat.OP_CONV and d.ksize == 5]
    assert len(k5) == 2 and all(d.stride == 2 for d in k5)
    assert (k5[0].cin, k5[0].cout, ch(k5[0].out_t), k5[0].in_t) == (8, 50, 56, pack.out_t)
    assert (k5[1].cin, k5[1].cout, k5[1].out_t, k5[1].out_coff, k5[1].reserved[2]) == (56, P, cat2, P + 8, P)
    w = np.frombuffer(p.blob, np.float16, 50 * 8 * 25, k5[0].w_off).reshape(50, 8, 25)
    assert not w[:, 3:].any() and w[:, :3].any(axis=(0, 2)).all()
    w = np.frombuffer(p.blob, np.float16, P * 56 * 25, k5[1].w_off).reshape(P, 56, 25)
    assert not w[:, 50:].any() and w[:, :50].any(axis=(0, 2)).all()
    # the attention CAMs read cat1's 51 logical channels, the pads get zero weights; slices of 16 (12 used) x 4 at P = 48
    hc, hp = (P + 3) // 4, -(-((P + 3) // 4) // 8) * 8
    readers = [d for d in p.ops if d.kind == nat.OP_CONV and d.in_t == cat1]
    assert len(readers) == 5 and all(d.cin == P + 8 for d in readers)          # residual + four dilations (att_hi)
    for d in readers:
        w = np.frombuffer(p.blob, np.float16, d.cout * d.cin * d.ksize ** 2, d.w_off).reshape(d.cout, d.cin, -1)
        assert not w[:, P + 3:].any() and w[:, :P + 3].any(axis=(0, 2)).all()
    slices = [d for d in readers if d.ksize == 3]
    assert sorted((d.reserved[1], d.out_coff, d.reserved[2]) for d in slices) == [(i + 1, hp * i, hp) for i in range(4)]
    assert all(ch(d.out_t) == 4 * hp for d in slices) and (P != 48 or (hc, hp) == (12, 16))
    # steps[0] reads cat2 through the column map: zero weights at the five pads
    pads = list(range(P + 3, P + 8))
    readers2 = [d for d in p.ops if d.kind == nat.OP_CONV and d.in_t == cat2]
    assert len(readers2) == 4 and all(d.cin == 2 * P + 8 for d in readers2)    # residual + three dilations
    for d in readers2:
        w = np.frombuffer(p.blob, np.float16, d.cout * d.cin * d.ksize ** 2, d.w_off).reshape(d.cout, d.cin, -1)
        assert not w[:, pads].any() and np.delete(w, pads, 1).any(axis=(0, 2)).all()
    se2 = [d for d in p.ops if d.kind == nat.OP_SE and d.in_t == cat2][0]
    w1 = np.frombuffer(p.blob, np.float32, se2.cout * se2.cin, se2.w_off).reshape(se2.cout, se2.cin)
    assert se2.cin == 2 * P + 8 and not w1[:, pads].any() and np.delete(w1, pads, 1).any(axis=0).all()
    # one program per divisor: without one the op carries 0
    q = m.compile_program(("att_divisor", None))
    assert [d for d in q.ops if d.kind == nat.OP_GATE_MUL][0].reserved[0] == 0 and H.program_rows(q) == H.program_rows(p)


def test_builder_keeps_the_fp32_forms_by_default_and_refuses_half_forms_in_an_fp32_program():
    from rtpe import _native as nat
    from rtpe.third_party.pose_higher_hrnet import ProgramBuilder
    b = ProgramBuilder(f32=False)
    a = b.aux_input()
    assert b.tensors[a] == [4, 0, 4] and b.ops[-1].flags & nat.F_F32 and b.ops[-1].cout == 4
    h = b.aux_input(half=True)
    assert b.tensors[h] == [8, 0, 2] and not b.ops[-1].flags & nat.F_F32 and b.ops[-1].cout == 8
    with pytest.raises(ValueError):
        ProgramBuilder(f32=True).aux_input(half=True)


# --------------------------------------------------------------------------- #
# (3) fixture, build
# --------------------------------------------------------------------------- #
def test_fixture_is_finite_fp16_and_its_spread_matches_its_arrays():
    g = np.load(os.path.join(GOLDEN, "steps_half.npz"))
    assert len(g.files) == 8 * len(STEPS_HALF_CASES)
    for name, P, _, n, h, w, _, _, _ in STEPS_HALF_CASES:
        for key, c in (("att", 1), ("det", 18)):
            a, b, r = (g["%s_%s_%s" % (name, key, k)] for k in ("half", "alt", "f32"))
            assert a.dtype == np.float16 and b.dtype == np.float16 and r.dtype == np.float32
            assert a.shape == b.shape == r.shape == (n, c, -(-h // 4), -(-w // 4))
            assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(r).all()
            d = np.abs(a.astype(np.float32) - b.astype(np.float32))
            sp = g["%s_%s_spread" % (name, key)]
            assert sp.shape == (2,) and float(d.max()) == sp[0] and abs(float(d.mean()) - sp[1]) <= 1e-9
            e = np.abs(a.astype(np.float32) - r)
            print("%s %s: spread max %.3e mean %.3e; half vs fp32 max %.3e mean %.3e" % (name, key, sp[0], sp[1], e.max(), e.mean()))
            assert e.max() <= 2e-3
    assert os.path.getsize(os.path.join(GOLDEN, "steps_half.npz")) < 1 << 20


def test_fp16_rounding_points_of_the_new_forms_survive_the_compiler(tmp_path):
    """as tests/test_student_half_host.py asks of the other four ops: no operation fused with the conversion behind it, and
    the fp16 and fp32 instantiations of the three kernels are in the object (the resize: one fp16 form, not mixed)"""
    import re
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    from test_host_logic import _device_code
    dis = _device_code(_native, tmp_path, "student_ops.hip")
    assert not re.findall(r"v_fma_mix(?:lo|hi)_f16", dis)
    for kernel in ("gate_mul_kernel", "aux_pack_kernel"):
        assert re.search(r"<_ZN4rtpe\d+%sIDF16_E" % kernel, dis) and re.search(r"<_ZN4rtpe\d+%sIfE" % kernel, dis), kernel
    for inst in ("ILb0EDF16_E", "ILb0EfE", "ILb1EfE"):
        assert re.search(r"<_ZN4rtpe\d+resize_nhwc_kernel%s" % inst, dis), inst
    assert not re.search(r"resize_nhwc_kernelILb1EDF16_", dis)
