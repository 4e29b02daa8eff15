"""The order-independent conv data of oracle/exact.py, checked on the CPU.

(1) Order independence: on this data PyTorch-CPU's fp32 convolution gives the float64 result bit for bit with oneDNN
    on, with oneDNN off and with the input channels permuted - three accumulation orders nobody controls - and the
    BatchNorm value is an fp32 number.  So the expected output of tests/test_conv_exact_gpu.py is THE answer for any
    kernel that accumulates in fp32, not one implementation's.
(2) The data can see faults: each seeded fault of ``exact.MUTATIONS``, applied to the reference, changes at least one
    output element in every (class, regime) where it applies.  Where a fault cannot apply it is not silently passed:
    ``applies`` states the rule, and the test asserts that the fault is indeed invisible there only because the data
    holds nothing for it to act on.
(3) The sibling sets of the grouped stride-2 launch (conv48s2_launch_group): their chains stay inside the exact range,
    and nine seeded faults of the launch's per-slot bookkeeping each change every sibling they act on.

The case tables and the layer builders of the GPU file live here, so that both files walk the same list."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import exact
from test_gpu_parity import CONV_CASES, FP32_CONV_CASES

torch.set_num_threads(min(16, torch.get_num_threads()))

# every (cin, cout, k, stride) of the network's conv layers, in CONV_CASES' order
CLASSES = list(dict.fromkeys(c[:4] for c in CONV_CASES))
SEED = 20240


def regimes_of(cls):
    """`overflow` on 48 -> 48 and 384 -> 384 only (a BasicBlock's convs: the layers with a residual behind them)"""
    return ("int", "denorm", "cancel") + (("overflow",) if cls in ((48, 48, 3, 1), (384, 384, 3, 1)) else ())


# the fp32 classes of the GPU list: FP32_CONV_CASES' (cin, cout, k, stride, dilation) and the students' 5x5 stride-2 conv
F32_CLASSES = list(dict.fromkeys(c[:5] for c in FP32_CONV_CASES)) + [(32, 32, 5, 2, 1)]
CLASS_REGIMES = [(cls, r) for cls in CLASSES for r in regimes_of(cls)]
_ID = lambda v: "%d-%d_k%ds%d" % v if isinstance(v, tuple) else str(v)


def seed_of(cls, regime, shape=(0, 0, 0)):
    return SEED + 7 * cls[0] + 13 * cls[1] + cls[2] + cls[3] + exact.REGIMES.index(regime) * 1009 + shape[1] * 31 + shape[2]


# --------------------------------------------------------------------------- #
# programs: layers with exact data (the program tests of tests/test_conv_exact_gpu.py build them into executors)
# --------------------------------------------------------------------------- #
def _layer(cin, cout, k, s, g, bn=True, alpha_choices=(0.5, 1.0), density=1.0):
    """a Conv2d (+ BatchNorm2d that folds to exactly alpha, beta) with weights in {-1, 0, 1}; alpha a power of two and beta
    a multiple of 1/2, so the quantum of the activations halves per layer at the most.  ``density`` < 1 keeps that share
    of the weights and zeroes the others: the sums of a deep chain grow more slowly"""
    import torch.nn as nn
    conv = nn.Conv2d(cin, cout, k, s, k // 2, bias=not bn)
    w = torch.randint(-1, 2, conv.weight.shape, generator=g).float()
    if density < 1.0:
        w = w * (torch.rand(w.shape, generator=g) < density)
    alpha = torch.tensor(alpha_choices)[torch.randint(0, len(alpha_choices), (cout,), generator=g)] if bn else torch.ones(cout)
    beta = torch.randint(-8, 9, (cout,), generator=g).float() / 2
    norm = None
    with torch.no_grad():
        conv.weight.copy_(w)
        if bn:
            norm = nn.BatchNorm2d(cout)
            norm.weight.copy_(alpha); norm.bias.copy_(beta); norm.running_mean.zero_(); norm.running_var.fill_(1.0 - norm.eps)
        else:
            conv.bias.copy_(beta)
    conv.half()
    return conv, norm, w.double(), alpha.double(), beta.double()


def _ref_layer(x, layer, k, s, relu, round_conv, res=None, quantum=None):
    """one layer of a program in float64; asserts the order-independence bound for its input"""
    conv, norm, w, alpha, beta = layer
    taps = w.shape[1] * k * k
    assert torch.equal(torch.round(x / quantum) * quantum, x) and taps * float(x.abs().max()) / quantum < 2 ** 24
    return exact.reference(x, w, alpha, beta, res, k, s, 1, relu, round_conv).out


# --------------------------------------------------------------------------- #
# sibling 3x3 stride-2 convs from one 48-channel map: the grouped launch of csrc/conv48s2.hip (conv48s2_launch_group)
# --------------------------------------------------------------------------- #
# (id, [(cout, relu, bn) per sibling], rtpe_hrnet_op_tile's marks under the default options): -(200000 + n) for the first op
# of a group of n, -200009 for the others, -200001 for a conv on a launch of its own
SIBLING_SETS = [
    ("96_48r", [(96, 0, 1), (48, 1, 1)], [-200002, -200009]),                        # the teacher's stage-3 pair: GW = 4, empty fourth slot
    ("96_48r_48r", [(96, 0, 1), (48, 1, 1), (48, 1, 1)], [-200003, -200009, -200009]),   # its stage-4 triple: four full slots
    ("48r_48", [(48, 1, 1), (48, 0, 1)], [-200002, -200009]),                        # GW = 2
    ("48r_96", [(48, 1, 1), (96, 0, 1)], [-200002, -200009]),                        # grp0 restarts at 0 in slot 1
    ("96r_96", [(96, 1, 1), (96, 0, 1)], [-200002, -200009]),                        # two layers of two groups
    ("48r_48_48r", [(48, 1, 1), (48, 0, 1), (48, 1, 1)], [-200003, -200009, -200009]),   # every slot another layer, empty fourth
    ("48_48r_48_48r", [(48, 0, 1), (48, 1, 1), (48, 0, 1), (48, 1, 1)], [-200003, -200009, -200009, -200001]),   # 3 layers at the most
    ("96r_96_48r", [(96, 1, 1), (96, 0, 1), (48, 1, 1)], [-200002, -200009, -200001]),   # 4 groups at the most
    ("96b_48rb", [(96, 0, 0), (48, 1, 0)], [-200002, -200009]),                      # bias only: the ROUND = false instantiation
    ("96_48rb", [(96, 0, 1), (48, 1, 0)], [-200001, -200001]),                       # F_ROUND_CONV differs: no group
]
SIBLING_IDS = [s_[0] for s_ in SIBLING_SETS]
SIBLING_SHAPES = [(3, 5), (9, 17), (23, 37)]            # the siblings' output sizes: below a tile, a pixel over one, ragged
# A forward takes inputs of multiples of 32 pixels, so a 3 x 5 map exists at 1 / 32 only: the small shapes run the `deep`
# front (stem, 64 -> 48 and twice 48 -> 48, all 3x3 stride 2: the siblings' input t at 1 / 16).  The walked case runs the
# shallow one (stem, conv 1x1 64 -> 48: t at 1 / 2, the siblings at 1 / 4): 20 images of 64 x 64 outputs are 1,280 units of
# 8 x 8 pixels (a group has one cout block), five for each of the 256 persistent workgroups, so that a workgroup's fifth
# halo tile lands in the buffer of its first (conv48s2.hip keeps four)
SIBLING_WALKED = (20, 64, 64)
SIBLING_WALKED_IDS = ["96_48r", "96_48r_48r", "48r_48"]     # one per GW instantiation and empty-slot variant
# what the GPU test fills the workspace with in front of every forward: an element a launch never writes holds this
SIBLING_PRESET = exact.IN_SENTINEL


def sibling_shapes(i):
    """(N, H, W) of set number i at the three small shapes: N goes 3, 1, 3 or 1, 3, 1 (as shapes_of in the GPU file)"""
    return [((3, 1)[(i + pos) % 2],) + s_ for pos, s_ in enumerate(SIBLING_SHAPES)]


def static_groups(sibs):
    """rtpe_hrnet_create's static rule on neighbouring siblings that share input, lane and region and have no residual: a
    run of up to three with the same F_ROUND_CONV (set where a layer has a BatchNorm) and four groups of 48 channels at
    the most; returns the lengths of the runs (1: a conv on its own)"""
    runs, i = [], 0
    while i < len(sibs):
        n, groups = 1, sibs[i][0] // 48
        while i + n < len(sibs) and n < 3 and sibs[i + n][2] == sibs[i][2] and groups + sibs[i + n][0] // 48 <= 4:
            groups += sibs[i + n][0] // 48
            n += 1
        runs.append(n)
        i += n
    return runs


def sibling_marks(sibs):
    return [m for n in static_groups(sibs) for m in ([-(200000 + n)] + [-200009] * (n - 1) if n > 1 else [-200001])]


@functools.lru_cache(maxsize=None)
def sibling_front_layers(deep):
    """stem and the convs (layer, k, stride) up to the 48-channel map t; the same for every sibling set.  One alpha per
    layer and thinned weights behind the stem keep max |activation| / quantum of t where the siblings' sums are exact
    (432 taps: below 2^24 / 432 quanta) and their conv values are mostly NOT fp16 numbers (beyond 2^11 quanta: the
    conv's own rounding, F_ROUND_CONV, is seen)"""
    g = torch.Generator().manual_seed(SEED + 4800 + deep)
    stem = _layer(3, 64, 3, 2, g)
    if not deep:
        return stem, [(_layer(64, 48, 1, 1, g, alpha_choices=(0.5,)), 1, 1)]
    return stem, [(_layer(64, 48, 3, 2, g, alpha_choices=(0.5,), density=0.25), 3, 2),
                  (_layer(48, 48, 3, 2, g, alpha_choices=(0.5,), density=0.125), 3, 2),
                  (_layer(48, 48, 3, 2, g, alpha_choices=(0.5,), density=0.125), 3, 2)]


@functools.lru_cache(maxsize=None)
def sibling_front(deep, N, Ho, Wo):
    """the fp16 input (N, 3, H, W) for siblings' outputs of Ho x Wo, the map t in float64 and its quantum"""
    scale = 32 if deep else 4
    g = torch.Generator().manual_seed(SEED + 131 * Ho + Wo + N)
    x = torch.randint(-3, 4, (N, 3, Ho * scale, Wo * scale), generator=g).half()
    stem, convs = sibling_front_layers(deep)
    t, q = _ref_layer(x.double(), stem, 3, 2, True, True, quantum=1.0), 0.5
    for layer, k, s in convs:
        t, q = _ref_layer(t, layer, k, s, True, True, quantum=q), q / 2
    return x, t, q


@functools.lru_cache(maxsize=None)
def sibling_layers(set_id):
    """the set's sibling layers: each its own weights, per-channel alpha in {1/2, 1} (1 without BatchNorm) and beta"""
    i = SIBLING_IDS.index(set_id)
    g = torch.Generator().manual_seed(SEED + 977 * (i + 1))
    return [_layer(48, cout, 3, 2, g, bn=bool(bn)) for cout, relu, bn in SIBLING_SETS[i][1]]


SIBLING_FAULTS = ("weights_swapped", "outputs_swapped", "affine_of_another", "second_group_first_weights",
                  "second_group_first_affine", "relu_of_neighbour", "last_slot_unwritten", "pitch_of_the_96", "conv_unrounded")


def sibling_fault_plan(sibs, fault):
    """Which siblings of the set's first run a seeded bookkeeping fault of the grouped launch acts on: (a, b) - the fault
    moves something from a to b, or between them, or acts on b alone - or None where the set holds nothing for it"""
    run = list(range(static_groups(sibs)[0])) if static_groups(sibs)[0] > 1 else list(range(len(sibs)))
    wide = [k for k in run if sibs[k][0] == 96]
    narrow = [k for k in run if sibs[k][0] == 48]
    if fault in ("weights_swapped", "outputs_swapped", "affine_of_another"):
        return run[0], run[1]
    if fault in ("second_group_first_weights", "second_group_first_affine"):
        return (wide[0], wide[0]) if wide else None
    if fault == "relu_of_neighbour":
        pairs = [(k, k + 1) for k in run[:-1] if sibs[k][1] != sibs[k + 1][1]]
        return pairs[0] if pairs else None
    if fault == "last_slot_unwritten":
        return run[-1], run[-1]
    if fault == "pitch_of_the_96":
        return (wide[0], narrow[0]) if wide and narrow else None
    if fault == "conv_unrounded":
        rounded = [k for k in run if sibs[k][2]]
        return (rounded[0], rounded[-1]) if rounded else None
    raise ValueError(fault)


def sibling_outputs(set_id, t, q, fault=None):
    """The float64 outputs (N, cout, H, W) of the set's siblings, computed the way the grouped launch is laid out: one
    slot per group of 48 output channels with its own weights, alpha / beta, ReLU flag, rounding flag, destination
    (sibling, first channel) and row pitch, written into NHWC buffers preset to SIBLING_PRESET through a window of the
    buffer's size.  Without a fault this is _ref_layer per sibling (asserted, with its bound on the input); ``fault``
    seeds one of SIBLING_FAULTS into the slot table, and the second value returned lists the siblings it must change"""
    sibs = SIBLING_SETS[SIBLING_IDS.index(set_id)][1]
    layers = sibling_layers(set_id)
    assert torch.equal(torch.round(t / q) * q, t) and 432 * float(t.abs().max()) / q < 2 ** 24
    convs = [F.conv2d(t, l[2], None, 2, 1) for l in layers]
    slots = [dict(w=(k, j), ab=(k, j), relu=sibs[k][1], rnd=sibs[k][2], dst=(k, j), pitch=sibs[k][0], skip=False)
             for k in range(len(sibs)) for j in range(sibs[k][0] // 48)]
    first = {k: next(s_ for s_ in slots if s_["dst"] == (k, 0)) for k in range(len(sibs))}
    hit = []
    if fault is not None:
        a, b = sibling_fault_plan(sibs, fault)
        sa, sb = first[a], first[b]
        second = next((s_ for s_ in slots if s_["dst"] == (b, 1)), None)
        hit = [b]
        if fault == "weights_swapped":
            sa["w"], sb["w"], hit = sb["w"], sa["w"], [a, b]
        elif fault == "outputs_swapped":
            sa["dst"], sb["dst"], sa["pitch"], sb["pitch"], hit = sb["dst"], sa["dst"], sb["pitch"], sa["pitch"], [a, b]
        elif fault == "affine_of_another":
            sb["ab"] = sa["ab"]
        elif fault == "second_group_first_weights":
            second["w"] = (b, 0)
        elif fault == "second_group_first_affine":
            second["ab"] = (b, 0)
        elif fault == "relu_of_neighbour":
            for s_ in slots:
                if s_["dst"][0] == b:
                    s_["relu"] = sibs[a][1]
        elif fault == "last_slot_unwritten":
            (second or sb)["skip"] = True
        elif fault == "pitch_of_the_96":
            sb["pitch"] = sibs[a][0]
        elif fault == "conv_unrounded":
            run = range(static_groups(sibs)[0]) if static_groups(sibs)[0] > 1 else range(len(sibs))
            hit = [k for k in run if sibs[k][2]]
            for s_ in slots:
                if s_["dst"][0] in hit:
                    s_["rnd"] = 0
    r16 = exact.round16 if fault is None else (lambda v: v.float().half().double())
    N, _, H, W = convs[0].shape
    bufs = [torch.full((N * H * W * c[0],), SIBLING_PRESET, dtype=torch.float64) for c in sibs]
    pix = torch.arange(N * H * W).view(-1, 1)
    for s_ in slots:
        if s_["skip"]:
            continue
        (kw, jw), (ka, ja), (kd, jd) = s_["w"], s_["ab"], s_["dst"]
        c = convs[kw][:, 48 * jw:48 * jw + 48]
        alpha, beta = (v[48 * ja:48 * ja + 48].view(1, -1, 1, 1) for v in layers[ka][3:5])
        v = r16((r16(c) if s_["rnd"] else c) * alpha + beta)
        if s_["relu"]:
            v = torch.where(v > 0, v, torch.zeros_like(v))
        at = pix * s_["pitch"] + 48 * jd + torch.arange(48).view(1, -1)          # the element offsets of the slot's stores
        ok = at < bufs[kd].numel()                                                # ... inside the buffer's window
        bufs[kd][at[ok]] = v.permute(0, 2, 3, 1).reshape(-1, 48)[ok]
    outs = [b_.view(N, H, W, c[0]).permute(0, 3, 1, 2).contiguous() for b_, c in zip(bufs, sibs)]
    if fault is None:
        for o, l, c in zip(outs, layers, sibs):
            assert torch.equal(o, _ref_layer(t, l, 3, 2, bool(c[1]), bool(c[2]), quantum=q))
        return outs
    return outs, hit


def smallest(cls, regime, **kw):
    """the case at the smallest GPU shape: one image with a 3 x 5 output"""
    cin, cout, k, s = cls
    args = dict(residual=True, relu=False, round_conv=True)
    args.update(kw)
    return exact.exact_case(cin, cout, k, s, 1, 1, 3 * s, 5 * s, regime, seed_of(cls, regime), **args)


def applies(mutation, cls, regime):
    cin, cout, k, s = cls
    if mutation == "halo_sentinel":            # a 3x3 stride-2 conv of an even-sized map never reads the row below it
        return k > 1 and s == 1
    if mutation == "flush_denormals":          # the other regimes hold no fp16 denormal
        return regime == "denorm"
    if mutation in ("conv_rtz", "conv_unrounded", "single_rounding"):
        # `int` and `overflow` convs and BatchNorm values are fp16 numbers already: these regimes pin indexing and
        # the overflow behaviour, `denorm` and `cancel` pin the rounding points
        return regime in ("denorm", "cancel")
    return True


@pytest.mark.parametrize("cls,regime", CLASS_REGIMES, ids=_ID)
def test_fp32_accumulation_is_exact_in_any_order(cls, regime):
    cin, cout, k, s = cls
    c = smallest(cls, regime)
    x, w, want = c.x64.float(), c.w64.float(), c.ref.conv
    perm = torch.randperm(cin, generator=torch.Generator().manual_seed(cin))
    got = {"oneDNN": F.conv2d(x, w, None, s, k // 2)}
    with torch.backends.mkldnn.flags(enabled=False):
        got["no oneDNN"] = F.conv2d(x, w, None, s, k // 2)
    got["permuted channels"] = F.conv2d(x[:, perm].contiguous(), w[:, perm].contiguous(), None, s, k // 2)
    for name, y in got.items():
        assert y.dtype == torch.float32 and torch.equal(y.double(), want), name
    # BatchNorm: the product-sum is an fp32 number, so fp32 arithmetic gives it whether fused or not
    bn32 = torch.addcmul(c.beta.view(1, -1, 1, 1), c.ref.conv_r.float(), c.alpha.view(1, -1, 1, 1))
    assert torch.equal(bn32.double(), c.ref.bn) and torch.equal(c.ref.bn.float().double(), c.ref.bn)
    assert torch.equal(c.alpha.double(), c.alpha64) and torch.equal(c.beta.double(), c.beta64)


@pytest.mark.parametrize("cls,regime", CLASS_REGIMES, ids=_ID)
def test_each_seeded_fault_changes_the_output(cls, regime):
    c = smallest(cls, regime)
    want = c.want.numpy().view(np.int16)
    for m in exact.MUTATIONS:
        got = smallest(cls, regime, mutate=m).want.numpy().view(np.int16)
        changed = int((got != want).sum())
        if applies(m, cls, regime):
            assert changed > 0, "%s goes unnoticed" % m
        else:
            assert changed == 0, "%s applies after all: say so in applies()" % m


@pytest.mark.parametrize("cin", [48, 96])
@pytest.mark.parametrize("regime", ["int", "denorm", "cancel"])
def test_transposed_conv_is_exact_in_any_order(cin, regime):
    """the k4 s2 p1 transposed conv of the GPU list (cin 48 and 96, 48 output channels) at its smallest shape"""
    c = exact.exact_case(cin, 48, 4, 2, 1, 1, 3, 5, regime, SEED + cin + exact.REGIMES.index(regime), False, False, True,
                         transposed=True)
    x, w, want = c.x64.float(), c.w64.float(), c.ref.conv
    perm = torch.randperm(cin, generator=torch.Generator().manual_seed(cin))
    got = {"oneDNN": F.conv_transpose2d(x, w, None, 2, 1)}
    with torch.backends.mkldnn.flags(enabled=False):
        got["no oneDNN"] = F.conv_transpose2d(x, w, None, 2, 1)
    got["permuted channels"] = F.conv_transpose2d(x[:, perm].contiguous(), w[perm].contiguous(), None, 2, 1)
    for name, y in got.items():
        assert y.shape == (1, 48, 6, 10) and torch.equal(y.double(), want), name
    assert torch.equal(c.ref.bn.float().double(), c.ref.bn)
    # the data sees the faults that apply to a transposed conv
    for m in ("skip_last_chunk",) + (("flush_denormals",) if regime == "denorm" else ()) + \
            (("conv_rtz", "conv_unrounded") if regime != "int" else ()):
        got = exact.exact_case(cin, 48, 4, 2, 1, 1, 3, 5, regime, SEED + cin + exact.REGIMES.index(regime), False, False, True,
                               transposed=True, mutate=m)
        assert not torch.equal(got.want.view(torch.int16), c.want.view(torch.int16)), m


@pytest.mark.parametrize("case", F32_CLASSES, ids=lambda c: "f32_%d-%d_k%ds%dd%d" % c)
def test_fp32_cases_hold_integers_below_2_to_24(case):
    cin, cout, k, s, dil = case
    c = exact.exact_case(cin, cout, k, s, dil, 1, 3 * s, 5 * s, "int", SEED + cin + dil, True, False, False, f32=True)
    for t in (c.ref.conv, c.ref.bn, c.ref.out):
        assert torch.equal(torch.round(t), t) and float(t.abs().max()) < 2 ** 24
    y = F.conv2d(c.x, c.w, None, s, dil * (k // 2), dil)
    assert torch.equal(y.double(), c.ref.conv)
    for m in ("drop_tap", "skip_last_chunk") + (("halo_sentinel",) if k > 1 and (s == 1 or k == 5) else ()):
        got = exact.exact_case(cin, cout, k, s, dil, 1, 3 * s, 5 * s, "int", SEED + cin + dil, True, False, False, f32=True,
                               mutate=m)
        assert not torch.equal(got.want, c.want), m


def test_the_regimes_reach_what_they_claim():
    for cls, regime in CLASS_REGIMES:
        c = smallest(cls, regime)
        out = c.want.float()
        if regime == "denorm":
            assert float(c.x.float().abs().max()) < 2.0 ** -14
            normal = (out.abs() >= 2.0 ** -14).float().mean().item()
            assert normal > 0.9, (cls, normal)
            rep = (c.ref.conv.float().half().double() == c.ref.conv).double().mean().item()
            assert rep < 0.75, (cls, rep)                 # a quarter and more of the conv values are NOT fp16 numbers
        if regime == "cancel":
            assert torch.isfinite(out).all()
        if regime == "overflow":
            assert torch.isinf(out).any() and torch.isfinite(out).any() and not torch.isnan(out).any()
            assert (out == float("inf")).any() and (out == -float("inf")).any()


def test_round_toward_zero_helper_and_guard_patterns():
    v = torch.tensor([1.0 + 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 2049.0, 0.5, -65519.0], dtype=torch.float64)
    assert exact.round16_toward_zero(v).tolist() == [1.0, -(1.0 + 2.0 ** -10), 2048.0, 0.5, -65504.0]
    assert exact.round16(v).tolist() == [1.0, -(1.0 + 2.0 ** -9), 2048.0, 0.5, -65504.0]
    for es, dt in ((2, torch.float16), (4, torch.float32)):
        idt = torch.int16 if es == 2 else torch.int32
        bits = exact.OUT_PATTERN[es]
        bits = bits - (1 << 8 * es) if bits >= 1 << (8 * es - 1) else bits
        assert torch.isnan(torch.tensor([bits], dtype=idt).view(dt)).all()
    assert np.isfinite(np.float16(exact.IN_SENTINEL))


# --------------------------------------------------------------------------- #
# the sibling sets of the grouped stride-2 launch
# --------------------------------------------------------------------------- #
def test_sibling_sets_group_as_the_static_rule_says():
    """the marks the GPU test expects from rtpe_hrnet_op_tile are what rtpe_hrnet_create's rule gives (static_groups is that
    rule in Python; creating an executor needs a GPU, so the rule itself is asserted on the labels in the GPU file)"""
    for set_id, sibs, marks in SIBLING_SETS:
        assert sibling_marks(sibs) == marks, set_id
        assert len(sibling_layers(set_id)) == len(sibs)
    assert [static_groups(s_[1]) for s_ in SIBLING_SETS] == [[2], [3], [2], [2], [2], [3], [3, 1], [2, 1], [2], [1, 1]]
    assert all(i in SIBLING_IDS for i in SIBLING_WALKED_IDS)
    N, Ho, Wo = SIBLING_WALKED
    assert N * (Ho // 8) * (Wo // 8) >= 5 * 256 and Ho % 8 == 0 and Wo % 8 == 0


@pytest.mark.parametrize("set_id", SIBLING_IDS)
def test_sibling_sets_are_exact_and_see_each_bookkeeping_fault(set_id):
    """On the layers and inputs of the GPU cases (the smallest shape of each set): the chain stays inside the exact range
    (_ref_layer's bound for every layer, in sibling_front and sibling_outputs), every ReLU clips something and leaves
    something, negative values survive in the plain siblings, and each fault of SIBLING_FAULTS changes at least one
    element of every sibling it acts on.  Where a set holds nothing for a fault, that is asserted too"""
    i = SIBLING_IDS.index(set_id)
    sibs = SIBLING_SETS[i][1]
    N, Ho, Wo = sibling_shapes(i)[0]
    x, t, q = sibling_front(True, N, Ho, Wo)
    assert x.shape == (N, 3, 32 * Ho, 32 * Wo) and t.shape == (N, 48, 2 * Ho, 2 * Wo)
    want = sibling_outputs(set_id, t, q)
    layers = sibling_layers(set_id)
    for o, l, (cout, relu, bn) in zip(want, layers, sibs):
        assert o.shape == (N, cout, Ho, Wo) and torch.isfinite(o).all() and torch.equal(o.half().double(), o)
        plain = exact.reference(t, l[2], l[3], l[4], None, 3, 2, 1, False, bool(bn)).out
        for g0 in range(0, cout, 48):                      # in every group of 48 channels
            assert (plain[:, g0:g0 + 48] < 0).any() and (plain[:, g0:g0 + 48] > 0).any()
            assert bool((o[:, g0:g0 + 48] < 0).any()) == (not relu)
        assert (l[1] is None) == (not bn) and l[3].unique().numel() == (2 if bn else 1) and l[4].unique().numel() > 4
    run = static_groups(sibs)[0]
    has96, has48 = any(c[0] == 96 for c in sibs[:max(run, 2)]), any(c[0] == 48 for c in sibs[:max(run, 2)])
    nothing_to_act_on = {"second_group_first_weights": not has96, "second_group_first_affine": not has96,
                         "pitch_of_the_96": not (has96 and has48), "conv_unrounded": not any(c[2] for c in sibs),
                         "relu_of_neighbour": len({c[1] for c in sibs}) == 1}
    for fault in SIBLING_FAULTS:
        if sibling_fault_plan(sibs, fault) is None:
            assert nothing_to_act_on[fault], "%s: no plan for %s" % (set_id, fault)
            continue
        got, hit = sibling_outputs(set_id, t, q, fault)
        assert hit, fault
        for k in range(len(sibs)):
            changed = int((got[k].half().view(torch.int16) != want[k].half().view(torch.int16)).sum())
            assert (changed > 0) == (k in hit), "%s: %s changes %d elements of sibling %d" % (set_id, fault, changed, k)
