"""The data and the float64 references of tests/test_student_ops_gpu.py, checked on the CPU.

(1) Each reference of oracle/student_ops.py equals the corresponding PyTorch-CPU fp32 op bit for bit on the data of the
    GPU cases: ``F.avg_pool2d``, ``F.interpolate`` (bilinear, align_corners=False) at every ratio, the ``SELayer`` /
    ``ContextAwareModule`` tail of rtpe/students.py up to the sigmoid, ``torch.cat`` for the channel ranges.
(2) The data can see faults: each seeded fault of ``student_ops.MUTATIONS`` changes at least one output element, or takes
    a sigmoid out of its budget, in every case where it applies.  Where a fault cannot apply, ``applies`` states the rule
    and the test asserts that the fault is indeed invisible there.
(3) The sigmoid budget (``4 + |argument|`` ulps, derived in oracle/student_ops.py): PyTorch's fp32 restatement
    ``1 / (1 + exp(-(l / div)))`` stays inside it on the very logits the GPU test uses, and each sigmoid fault leaves it.

The case tables and the data of the GPU file live here, so that both files walk the same lists."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import exact
from oracle import student_ops as so

torch.set_num_threads(min(16, torch.get_num_threads()))
SEED = 31337
D = torch.float64


def _g(*key):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


# --------------------------------------------------------------------------- #
# what the four product programs emit (listed from the compiled programs, not by hand)
# --------------------------------------------------------------------------- #
# NOTE: the parametrize lists of this file and of the GPU file are built from these programs, so the four students are
# compiled (on the CPU, about 1.5 s) while pytest collects either file, `-m "not gpu"` included: a failure in
# rtpe/students.py shows up as a collection error here.  That is the price of listing the shapes from the compiled programs.
@functools.lru_cache(maxsize=1)
def student_programs():
    from rtpe.students import AttentionStudent, AttentionStudentSteps
    return {"student100": AttentionStudent(None, "cpu", inplanes=100).compile_program(),
            "student48": AttentionStudent(None, "cpu", inplanes=48).compile_program(),
            "student64_f32": AttentionStudent(None, "cpu", inplanes=64, half_precision=False).compile_program(),
            "steps48": AttentionStudentSteps(None, "cpu", inplanes=48).compile_program()}


@functools.lru_cache(maxsize=1)
def emitted():
    """distinct (C, ld) of the avgpool ops, (C, hid, in_ld, zero columns of w1) of the SE ops and (C, in_ld, out_ld) of the
    casts of the four programs"""
    from rtpe import _native as nat
    pool, se, casts = [], [], []
    for p in student_programs().values():
        for d in p.ops:
            ld = p.tensors[d.in_t].channels if d.in_t >= 0 else 0
            if d.kind == nat.OP_AVGPOOL:
                pool.append((d.cin, ld))
                assert p.tensors[d.out_t].channels == ld
            if d.kind == nat.OP_CAST:
                casts.append((d.cin, ld, p.tensors[d.out_t].channels))
            if d.kind == nat.OP_SE:
                w1 = np.frombuffer(p.blob, np.float32, d.cin * d.cout, d.w_off).reshape(d.cout, d.cin)
                se.append((d.cin, d.cout, ld, tuple(np.nonzero((w1 == 0).all(0))[0].tolist())))
    uniq = lambda v: sorted(set(v))
    return types.SimpleNamespace(avgpool=uniq(pool), se=uniq(se), cast=uniq(casts))


# --------------------------------------------------------------------------- #
# feeds
# --------------------------------------------------------------------------- #
def make_layer(w, alpha, beta, stride):
    """an fp16 Conv2d + BatchNorm2d that folds to exactly (alpha, beta): the tuple test_conv_exact_gpu._ref_layer takes"""
    import torch.nn as nn
    cout, cin, k, _ = w.shape
    conv = nn.Conv2d(cin, cout, k, stride, k // 2, bias=False)
    norm = nn.BatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(w.float())
        norm.weight.copy_(alpha.float()); norm.bias.copy_(beta.float())
        norm.running_mean.zero_(); norm.running_var.fill_(1.0 - norm.eps)
    conv.half()
    return conv, norm, w.double(), alpha.double(), beta.double()


def ref_layer(x, layer, k, s, relu, quantum):
    """one fp16 layer in float64 with the half wrapper's rounding points; asserts the order-independence bound"""
    conv, norm, w, alpha, beta = layer
    taps = w.shape[1] * k * k
    assert torch.equal(torch.round(x / quantum) * quantum, x) and taps * float(x.abs().max()) / quantum < 2 ** 24
    return exact.reference(x, w, alpha, beta, None, k, s, 1, relu, True).out


@functools.lru_cache(maxsize=8)
def stem_feed(N, H, W):
    """x (N, 3, H, W) fp16 integers and the fp16 stem 3 -> 64 k3 s2 + ReLU (alpha a power of two): the map at 1/2 that the
    students cast to fp32; multiples of 1/2"""
    g = _g(1, N, H, W)
    x = _ints(g, -3, 3, (N, 3, H, W))
    w = _ints(g, -1, 1, (64, 3, 3, 3))
    alpha = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (64,), generator=g)].double()
    beta = _ints(g, -8, 8, (64,)) / 2
    stem = make_layer(w, alpha, beta, 2)
    y = ref_layer(x, stem, 3, 2, True, 1.0)
    return types.SimpleNamespace(x=x, stem=stem, out=y, quantum=0.5)


def sub_weights(cin_phys):
    """the k3 s2 conv that keeps the pixels at even positions of channels 0..2 (one centre tap each): 8 output channels"""
    w = torch.zeros(8, cin_phys, 3, 3, dtype=D)
    for c in range(3):
        w[c, c, 1, 1] = 1
    return w


def aux_feed(base, ds, g):
    """aux (N, 3, H, W) fp32 whose pixels at the multiples of 2^ds hold ``base`` (N, 3, H >> ds, W >> ds); every other pixel
    holds an integer that no weight of the ``ds`` sub-sampling convs reads.  Returns aux and the float64 map behind each
    conv: chain[0] is the packed aux (4 channels), chain[i] (8 channels, 3 used) sits at 1 / 2^i."""
    N, _, h, w = base.shape
    aux = _ints(g, -5, 5, (N, 3, h << ds, w << ds))
    aux[:, :, ::1 << ds, ::1 << ds] = base
    chain = [so.aux_pack(aux)]
    for i in range(ds):
        chain.append(so.exact_conv(chain[-1], sub_weights(chain[-1].shape[1]), None, 2))
    assert torch.equal(chain[-1][:, :3], base) and not chain[-1][:, 3:].any()
    return aux, chain


def mix_weights(g, cout, cin_phys, used=3, bias_amp=2):
    """integer 1x1 weights over the first ``used`` input channels, and an integer bias"""
    w = torch.zeros(cout, cin_phys, 1, 1, dtype=D)
    w[:, :used] = _ints(g, -1, 1, (cout, used, 1, 1))
    return w, _ints(g, -bias_amp, bias_amp, (cout,))


# --------------------------------------------------------------------------- #
# cast
# --------------------------------------------------------------------------- #
CAST_CASES = [(1, 32, 32), (3, 32, 32), (1, 96, 32), (3, 96, 32)]          # maps 16 x 16 and 48 x 16 behind the stem
CAST_SPECIALS = [65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, 0.0, 2.0 ** -14, -1023 * 2.0 ** -24]


@functools.lru_cache(maxsize=8)
def cast_data(N, H, W):
    """stem, then a 1x1 fp16 conv without ReLU whose power-of-two alphas scale the map into fp16 denormals, small and large
    normals; the first channels are constants (zero weights, beta): +-65504, the smallest denormals, zero"""
    f = stem_feed(N, H, W)
    g = _g(2, N, H, W)
    w = torch.zeros(64, 64, 1, 1, dtype=D)
    ns = len(CAST_SPECIALS)
    for c in range(ns, 64):
        idx = torch.randperm(64, generator=g)[:3]
        w[c, idx, 0, 0] = _ints(g, 0, 1, (3,)) * 2 - 1
    alpha = torch.tensor([2.0 ** -20, 2.0 ** -12, 1.0, 8.0])[torch.randint(0, 4, (64,), generator=g)].double()
    beta = torch.zeros(64, dtype=D)
    beta[:ns] = torch.tensor(CAST_SPECIALS, dtype=D)
    layer = make_layer(w, alpha, beta, 1)
    y = ref_layer(f.out, layer, 1, 1, False, f.quantum)
    want = so.cast(y)
    a = want.abs()
    assert ((a > 0) & (a < 2.0 ** -14)).any() and (want == 65504).any() and (want == -65504).any()
    assert (want < 0).any() and (want == 0).any() and torch.isfinite(want).all()
    return types.SimpleNamespace(feed=f, layer=layer, want=want)


# --------------------------------------------------------------------------- #
# avgpool
# --------------------------------------------------------------------------- #
# (N, H, W of the network input, ds of the pooled map, feed): maps 16 x 16 and 48 x 16 behind stem + cast, and 16 x 16 and 2 x 2
# behind the sub-sampled second input.  A program's tensors hold (H >> ds) x (W >> ds) pixels and inputs are multiples of 32, so
# a map with an odd side (2 x 1 and 1 x 1: the divisors 1 and 2) has no output tensor to pool into: the forward refuses it
# (AVGPOOL_REFUSED), and the reference is checked at those maps on the CPU alone.
AVGPOOL_MAPS = [(1, 32, 32, 1, "stem"), (3, 96, 32, 1, "stem"), (3, 32, 32, 1, "aux"), (3, 64, 64, 5, "aux")]
AVGPOOL_REFUSED = [(1, 64, 32, 5), (3, 32, 32, 5)]                  # maps 2 x 1 and 1 x 1


@functools.lru_cache(maxsize=4)
def avgpool_data(C, N, H, W, ds, feed):
    g = _g(3, C, N, H, W, ds)
    r = types.SimpleNamespace(kind=feed)
    if feed == "stem":
        r.feed = stem_feed(N, H, W)
        src, q = so.cast(r.feed.out), r.feed.quantum
        r.w, r.bias = mix_weights(g, C, 64, used=64, bias_amp=4)
    else:
        r.aux, r.chain = aux_feed(_ints(g, -9, 9, (N, 3, H >> ds, W >> ds)), ds, g)
        src, q = r.chain[-1], 1.0
        r.w, r.bias = mix_weights(g, C, 8, bias_amp=4)
    r.xin = so.exact_conv(src, r.w, r.bias, 1, False, q)
    r.ref = so.avgpool(r.xin)
    return r


# --------------------------------------------------------------------------- #
# SE gate + cam_combine
# --------------------------------------------------------------------------- #
SE_MAPS = {1: (32, 32, 5), 2: (64, 32, 5), 3: (96, 32, 5), 6: (96, 64, 5), 256: (32, 32, 1)}     # HW -> H, W, ds
SE_N = 3
SE_LARGE = [(264, 66, 264, ()), (512, 128, 512, ())]          # the second trip of the 256-thread loops; the kernel's limits
SE_REFUSED = [(520, 16, 520), (64, 129, 64)]                  # beyond them: an error return, not a launch


def se_cases():
    """(C, hid, in_ld, zero columns, HW): every emitted combination at HW 1 and 6, the first one at every HW, the large ones
    at HW 6 and 256"""
    out = []
    for i, c in enumerate(emitted().se):
        out += [c + (hw,) for hw in ((1, 2, 3, 6, 256) if i == 0 else (1, 6))]
    for c in SE_LARGE:
        out += [c + (6,), c + (256,)]
    return out


@functools.lru_cache(maxsize=4)
def se_data(C, hid, in_ld, zero_cols, HW):
    """the map is a per-image, per-channel constant plus a spatial pattern that sums to zero: integer means, both layers
    and the logit exact.  Gate channels by c % 4: logit 0 (gate 0.5), logit >= 20 (gate 1), logit <= -110 (gate 0), and
    generic integer logits with |l| <= 80 (judged by the budget)."""
    H, W, ds = SE_MAPS[HW]
    g = _g(4, C, hid, in_ld, HW)
    h, w = H >> ds, W >> ds
    const = _ints(g, -2, 2, (SE_N, 3, 1, 1))
    const[1] = const[0] + torch.tensor([1.0, -1.0, 2.0]).view(3, 1, 1)          # no two images alike
    base = const + so.zero_sum_pattern(h, w, 3, g)
    r = types.SimpleNamespace(N=SE_N, H=H, W=W, ds=ds, C=C, hid=hid, in_ld=in_ld)
    r.aux, r.chain = aux_feed(base, ds, g)
    r.wx, r.bx = mix_weights(g, in_ld, 8)
    r.x = so.exact_conv(r.chain[-1], r.wx, r.bx)                 # (N, in_ld, h, w): the pad channels hold data too
    c_out = C - len(zero_cols)                                   # the re-indexed form: fc2 is narrower than the row
    r.w1 = _ints(g, -1, 1, (hid, C))
    r.w1[:, list(zero_cols)] = 0
    r.b1 = _ints(g, -3, 3, (hid,))
    r.w2, r.b2 = torch.zeros(c_out, hid, dtype=D), torch.zeros(c_out, dtype=D)
    cls = torch.arange(c_out) % 4
    cls[-1] = 1                                                  # the last channel's gate is 1: a gate left at zero shows
    some = (torch.rand(c_out, hid, generator=g) < 0.3).double()
    r.w2[cls == 1], r.b2[cls == 1] = some[cls == 1], 20.0
    r.w2[cls == 2], r.b2[cls == 2] = -some[cls == 2], -110.0
    for c in torch.nonzero(cls == 3).flatten().tolist():
        idx = torch.randperm(hid, generator=g)[:2]
        r.w2[c, idx] = _ints(g, 0, 1, (2,)) * 2 - 1
        r.b2[c] = float(_ints(g, -3, 3, (1,)))
    w2p = torch.cat([r.w2, torch.zeros(C - c_out, hid, dtype=D)])
    b2p = torch.cat([r.b2, torch.zeros(C - c_out, dtype=D)])
    ref = so.se_gate(r.x[:, :C], r.w1, r.b1, w2p, b2p)
    wild = ((ref.logit.abs() > so.SIG_BAND) & (cls_pad(cls, C) == 3)).any(0)           # a generic logit outside the band:
    r.w2[wild[:c_out]] = 0                                                          # that channel keeps its bias alone
    w2p = torch.cat([r.w2, torch.zeros(C - c_out, hid, dtype=D)])
    r.w2p, r.b2p = w2p, b2p
    r.ref = so.se_gate(r.x[:, :C], r.w1, r.b1, w2p, b2p)
    generic = cls_pad(cls, C) == 3
    assert float(r.ref.logit[:, generic].abs().max()) <= so.SIG_BAND
    # a second combine on integers: the exact gates make it exact end to end, the generic ones one rounding each
    r.gl = (C + 7) // 8 * 8                                      # the width of the gate row and of the combine's operands
    r.w_res, r.b_res = mix_weights(g, r.gl, 8, bias_amp=6)
    r.w_hdc, r.b_hdc = mix_weights(g, r.gl, 8, bias_amp=6)
    r.res, r.hdc = so.exact_conv(r.chain[-1], r.w_res, r.b_res), so.exact_conv(r.chain[-1], r.w_hdc, r.b_hdc)
    return r


def cls_pad(cls, C):
    return torch.cat([cls, torch.full((C - cls.numel(),), -1, dtype=cls.dtype)])


def gate_row(gate, ld):
    """the gate row as the kernel leaves it: C gates, then zeros up to the row's width"""
    return torch.cat([gate, torch.zeros(gate.shape[0], ld - gate.shape[1], dtype=D)], 1)


# --------------------------------------------------------------------------- #
# sigmoid_add, gate_mul
# --------------------------------------------------------------------------- #
SIG_DIVS = (None, 20.0, 7.5)
SIGMOID_ADD_CASES = [(48, None), (104, None)]          # C; the op always divides by 20
GATE_MUL_CASES = [(P, div, order) for P, div in ((8, None), (8, 20.0), (8, 7.5), (48, 7.5)) for order in ("before", "after")]
SIG_SHAPE = (3, 32, 32)


@functools.lru_cache(maxsize=4)
def sig_data(C, div, tag=0):
    """the second input carries the integer logits in its first plane and small integers in the other two: the logits
    reach the op through a 1x1 selection, the gated tensor through a 1x1 integer mix"""
    N, H, W = SIG_SHAPE
    g = _g(5, C, int((div or 0) * 2), tag)
    l = so.logits_for(div, N * H * W, SEED + C + int((div or 0) * 2)).view(N, 1, H, W)
    aux = torch.cat([l, _ints(g, -9, 9, (N, 2, H, W))], 1)
    r = types.SimpleNamespace(N=N, H=H, W=W, aux=aux, logits=l, packed=so.aux_pack(aux))
    r.w_l = torch.zeros(1, 4, 1, 1, dtype=D)
    r.w_l[0, 0] = 1
    r.w_x = torch.zeros(C, 4, 1, 1, dtype=D)
    r.w_x[:, 1:3] = _ints(g, -1, 1, (C, 2, 1, 1))
    r.b_x = _ints(g, -4, 4, (C,))
    r.x = so.exact_conv(r.packed, r.w_x, r.b_x)
    return r


# --------------------------------------------------------------------------- #
# aux_pack, resize
# --------------------------------------------------------------------------- #
AUX_PACK_CASES = [(1, 32, 32), (3, 32, 32), (1, 96, 64), (3, 96, 64)]
# (source ds, target ds): ratios 4 (the product's), 2, 8, 1 (the shortcut), and the upscales 1/2 and 1/4
RESIZE_RATIOS = [(0, 2), (0, 1), (0, 3), (0, 0), (1, 0), (2, 0)]
RESIZE_CASES = [(s, t, N, H, W, order) for (s, t) in RESIZE_RATIOS for (N, H, W, order) in ((1, 32, 96, "before"), (3, 32, 96, "after"))]
RESIZE_P = 8


@functools.lru_cache(maxsize=4)
def aux_pack_data(N, H, W):
    g = _g(6, N, H, W)
    aux = (torch.randn(N, 3, H, W, generator=g) * 3).float().double()
    aux[:, :, 0, 0] = torch.tensor([0.0, -0.0, 1e30])            # zeros and a large value; no denormals
    assert float(aux[aux != 0].abs().min()) > 2.0 ** -126
    return types.SimpleNamespace(aux=aux, want=so.aux_pack(aux))


@functools.lru_cache(maxsize=4)
def resize_data(src_ds, tgt_ds, N, H, W):
    """the resized source is the second input itself (ds 0) or a sub-sampled copy of it; the target's other channels come
    from a 1x1 integer mix of the map at the target's resolution"""
    g = _g(7, src_ds, tgt_ds, N, H, W)
    top = max(src_ds, tgt_ds)
    aux, chain = aux_feed(_ints(g, -50, 50, (N, 3, H >> top, W >> top)), top, g)
    r = types.SimpleNamespace(N=N, H=H, W=W, aux=aux, chain=chain, top=top)
    r.src = chain[src_ds][:, :4]
    r.w_n, r.b_n = mix_weights(g, RESIZE_P, chain[tgt_ds].shape[1], bias_amp=9)
    r.neigh = so.exact_conv(chain[tgt_ds], r.w_n, r.b_n)
    r.ref = so.resize(r.src, H >> tgt_ds, W >> tgt_ds)
    r.want = torch.cat([r.neigh, r.ref.out], 1)
    return r


def resize_expect(src_ds, tgt_ds):
    """(the clamp at 0 acts, the last-row edge acts, the shortcut is taken) per ratio"""
    if src_ds == tgt_ds:
        return False, False, True
    up = src_ds > tgt_ds
    return up, up, False


# --------------------------------------------------------------------------- #
# the one large case: every grid-stride loop takes a second trip
# --------------------------------------------------------------------------- #
LARGE = (5, 512, 512)
ONE_TRIP = 4096 * 256


def large_items(N, H, W, C=64):
    """work items per grid-stride kernel of the large program (float4s; pixels for aux_pack), from the shapes"""
    h1, w1 = H // 2, W // 2
    return {"aux_pack": N * H * W, "resize": N * H * W * (4 // 4), "cast": N * h1 * w1 * (64 // 4),
            "cam_combine": N * h1 * w1 * (C // 4), "sigmoid_add": N * h1 * w1 * (C // 4),
            "gate_mul": N * h1 * w1 * (C // 4), "avgpool": N * (h1 // 2) * (w1 // 2) * (C // 4)}


# --------------------------------------------------------------------------- #
# (1) the references are PyTorch's fp32 ops
# --------------------------------------------------------------------------- #
def _bits(t):
    return t.float().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def test_the_programs_emit_what_the_tables_cover():
    e = emitted()
    assert len(e.avgpool) >= 4 and len(e.se) >= 6
    assert any(z for _, _, _, z in e.se), "the re-indexed w1 of emit(col_map=...) is gone"
    assert all(c == ld == out for c, ld, out in e.cast), "a cast with ld > C: add it to the cast cases"
    assert all(c <= 512 and hid <= 128 for c, hid, _, _ in e.se)


@pytest.mark.parametrize("hw", [(1, 1), (2, 1), (1, 3), (16, 12), (16, 16)], ids=lambda s: "%dx%d" % s)
def test_avgpool_reference_is_torch_fp32(hw):
    x = _ints(_g(8, *hw), -300, 300, (2, 5, hw[0], hw[1]))
    assert _same_bits(so.avgpool(x).out, F.avg_pool2d(x.float(), 3, 2, 1, count_include_pad=False))


def test_avgpool_cases_are_torch_fp32_and_reach_every_divisor():
    counts = set()
    for C, _ in emitted().avgpool:
        for m in AVGPOOL_MAPS:
            d = avgpool_data(C, *m)
            assert _same_bits(d.ref.out, F.avg_pool2d(d.xin.float(), 3, 2, 1, count_include_pad=False)), (C, m)
            if C == emitted().avgpool[0][0]:
                counts |= set(d.ref.counts)
    assert counts == {4, 6, 9}
    # the divisors 1 and 2 belong to maps with an odd side, which no program can hold: the reference alone, here
    for hw, cnt in (((1, 1), [1]), ((2, 1), [2]), ((1, 3), [2]), ((3, 3), [4])):
        x = _ints(_g(11, *hw), -300, 300, (2, 4, hw[0], hw[1]))
        r = so.avgpool(x)
        assert r.counts == cnt and _same_bits(r.out, F.avg_pool2d(x.float(), 3, 2, 1, count_include_pad=False))


@pytest.mark.parametrize("case", [c for c in RESIZE_CASES if c[5] == "before" or c[2] == 3], ids=str)
def test_resize_reference_is_torch_fp32(case):
    s, t, N, H, W, _ = case
    d = resize_data(s, t, N, H, W)
    got = F.interpolate(d.src.float(), (H >> t, W >> t), mode="bilinear", align_corners=False)
    assert _same_bits(d.ref.out, got)
    clamp0, edge, shortcut = resize_expect(s, t)
    for ax in (d.ref.y, d.ref.x):
        assert (ax.clamp0, ax.edge, ax.shortcut) == (clamp0, edge, shortcut), case
    # the channel range: torch.cat of the conv's channels and the resized ones
    assert torch.equal(so.place(torch.cat([d.neigh, torch.zeros_like(d.ref.out)], 1), RESIZE_P, d.ref.out), d.want)


@pytest.mark.parametrize("case", se_cases(), ids=lambda c: "C%d_hid%d_ld%d_z%d_hw%d" % (c[0], c[1], c[2], len(c[3]), c[4]))
def test_se_and_cam_references_are_the_torch_fp32_tail(case):
    d = se_data(*case)
    C = d.C
    x = d.x[:, :C].float()
    mean = x.mean((2, 3))                                            # AdaptiveAvgPool2d(1).view(b, c)
    h = F.relu(F.linear(mean, d.w1.float(), d.b1.float()))
    logit = F.linear(h, d.w2p.float(), d.b2p.float())
    assert torch.equal(logit.double(), d.ref.logit) and torch.equal(mean.double(), d.ref.mean)
    # the combine on the exact gates (0, 0.5, 1): F.relu(res + hdc * gate) in fp32
    gate = d.ref.gate.clone()
    gate[~so.sigmoid_map(d.ref.logit).exact] = 0.5
    want = F.relu(d.res[:, :C].float() + d.hdc[:, :C].float() * gate.float()[:, :, None, None])
    assert _same_bits(so.cam_combine(d.res[:, :C], d.hdc[:, :C], gate), want)
    # every gate class is there, and no two images share their generic gates
    s = so.sigmoid_map(d.ref.logit)
    assert (d.ref.gate == 0.5).any() and (d.ref.gate == 1).any() and (d.ref.gate == 0).any() and (~s.exact).any()
    assert not torch.equal(d.ref.logit[0], d.ref.logit[1]) and not torch.equal(d.ref.logit[0], d.ref.logit[2])


@pytest.mark.parametrize("case", AUX_PACK_CASES, ids=str)
def test_aux_pack_reference_is_a_cat(case):
    d = aux_pack_data(*case)
    assert _same_bits(d.want, torch.cat([d.aux.float(), torch.zeros(case[0], 1, case[1], case[2])], 1))
    assert not torch.signbit(d.want[:, 3]).any()


def test_cast_cases_reach_what_they_claim():
    for c in CAST_CASES:
        d = cast_data(*c)
        assert torch.equal(d.want.half().float().double(), d.want)


# --------------------------------------------------------------------------- #
# (3) the sigmoid budget
# --------------------------------------------------------------------------- #
def _torch_sigmoid32(l, div):
    a = l.float() / div if div else l.float()
    return 1.0 / (1.0 + torch.exp(-a))


@pytest.mark.parametrize("div", SIG_DIVS, ids=str)
def test_torch_fp32_restatement_is_inside_the_sigmoid_budget(div):
    for C in (8, 48, 104):
        l = sig_data(C, div).logits
        got = _torch_sigmoid32(l, div)
        ok, ulps, at, share, wrong = so.sigmoid_check(got, l, div)
        print("div %s: %.2f ulps at argument %.2f, %.0f %% of the budget, %d wrong exact points" % (div, ulps, at, 100 * share, wrong))
        assert ok
        s = so.sigmoid_map(l, div)
        assert (s.want == 0.5).any() and (s.want == 1).any() and (s.want == 0).any() and (~s.exact).sum() > 1000
    # the three exact points in fp32
    for a, v in ((0.0, 0.5), (18.0, 1.0), (-104.0, 0.0)):
        assert float(_torch_sigmoid32(torch.tensor([a]), None)) == v


@pytest.mark.parametrize("div", SIG_DIVS, ids=str)
def test_each_sigmoid_fault_leaves_the_budget(div):
    l = sig_data(8, div).logits
    for m in so.MUTATIONS["sigmoid_map"]:
        got = so.sigmoid_map(l, div, mutate=m).want.float()
        ok = so.sigmoid_check(got, l, div)[0]
        if sigmoid_fault_applies(m, div):
            assert not ok, "%s goes unnoticed" % m
        else:
            assert ok and torch.equal(so.sigmoid_arg(l, div, m), so.sigmoid_arg(l, div)), "%s applies after all" % m


def sigmoid_fault_applies(mutation, div):
    if mutation == "div_ignored":              # nothing to ignore where no division was asked
        return div is not None
    return div is None                         # div20_unasked: a case with a divisor of its own is divided by that one


# --------------------------------------------------------------------------- #
# (2) the data sees the seeded faults
# --------------------------------------------------------------------------- #
def test_each_avgpool_fault_changes_the_output():
    for C, _ in emitted().avgpool:
        for mp in AVGPOOL_MAPS:
            d = avgpool_data(C, *mp)
            h, w = d.xin.shape[2:]
            for m in so.MUTATIONS["avgpool"]:
                changed = not torch.equal(so.avgpool(d.xin, mutate=m).out, d.ref.out)
                assert changed == avgpool_fault_applies(m, h, w), (m, C, mp)


def avgpool_fault_applies(mutation, h, w):
    if mutation == "div9":                     # (a 1 x 1 .. 2 x 2 map has no window with nine taps inside, so it always applies)
        return True
    return max(h, w) > 2                       # shifted: the one window of a map of up to 2 x 2 holds the same pixels


@pytest.mark.parametrize("case", se_cases(), ids=lambda c: "C%d_hid%d_ld%d_z%d_hw%d" % (c[0], c[1], c[2], len(c[3]), c[4]))
def test_each_se_and_cam_fault_is_seen(case):
    d = se_data(*case)
    C, HW = d.C, case[4]
    for m in so.MUTATIONS["se_gate"]:
        got = so.se_gate(d.x[:, :C], d.w1, d.b1, d.w2p, d.b2p, mutate=m).gate.float()
        ok = so.sigmoid_check(got, d.ref.logit)[0]
        if m == "mean_short" and HW == 1:      # one pixel: a loop that ends one early has no mean at all (not modelled)
            assert ok
        else:
            assert not ok, "%s goes unnoticed" % m
    gate = d.ref.gate.float().double()
    want = so.cam_combine(d.res[:, :C], d.hdc[:, :C], gate)
    for m in so.MUTATIONS["cam_combine"]:
        assert not torch.equal(so.cam_combine(d.res[:, :C], d.hdc[:, :C], gate, mutate=m), want), m
    # the gate read through the combine with res = 0 and hdc = 1 is the gate
    assert torch.equal(so.cam_combine(torch.zeros_like(d.res[:, :C]), torch.ones_like(d.res[:, :C]), gate),
                       gate[:, :, None, None].expand_as(d.res[:, :C]))


@pytest.mark.parametrize("case", [c for c in RESIZE_CASES if c[2] == 3], ids=str)
def test_each_resize_fault_changes_the_output(case):
    s, t, N, H, W, _ = case
    d = resize_data(s, t, N, H, W)
    for m in so.MUTATIONS["resize"]:
        changed = not torch.equal(so.resize(d.src, H >> t, W >> t, mutate=m).out, d.ref.out)
        assert changed == resize_fault_applies(m, s, t), (m, case)
    # a store that runs one channel on lands in the next pixel's first channel: one of the conv's
    base = torch.cat([d.neigh, torch.zeros_like(d.ref.out)], 1)
    assert not torch.equal(so.place(base, RESIZE_P, d.ref.out, mutate="one_too_many"), d.want)
    assert not (d.neigh == so.SPILL_MARK).any()


def resize_fault_applies(mutation, src_ds, tgt_ds):
    if mutation == "no_clamp0":
        # never: real >= -0.5, so the truncation gives index 0 and the negative weight is caught by the clamp of lambda
        # to [0, 1] - dropping the clamp at 0 ALONE changes nothing in this kernel or in PyTorch's
        return False
    if mutation == "no_clamps":                # the clamps act on upscales only
        return src_ds > tgt_ds
    if mutation == "swapped_weights":
        # every power-of-two downscale has the weight 0.5 at every pixel of both axes and ratio 1 has (1, 0); the
        # weights of an upscale alternate along an axis
        return src_ds > tgt_ds
    return src_ds != tgt_ds                    # align_corners: the identity at ratio 1 either way


@pytest.mark.parametrize("case", AUX_PACK_CASES[1::2], ids=str)
def test_each_aux_pack_fault_changes_the_output(case):
    d = aux_pack_data(*case)
    for m in so.MUTATIONS["aux_pack"]:
        assert not torch.equal(so.aux_pack(d.aux, mutate=m), d.want), m


@pytest.mark.parametrize("case", GATE_MUL_CASES[::2], ids=str)
def test_gate_mul_channel_range_sees_a_store_too_far(case):
    P, div, _ = case
    d = sig_data(P + 4, div, 1)
    att = so.sigmoid_map(d.logits, div).want.float().double()
    neigh = so.exact_conv(d.packed, *gate_mul_neighbour(P))
    base = torch.cat([torch.zeros_like(d.x), neigh], 1)
    want = torch.cat([so.gate_mul(d.x, att), neigh], 1)
    assert torch.equal(so.place(base, 0, so.gate_mul(d.x, att)), want)
    assert not torch.equal(so.place(base, 0, so.gate_mul(d.x, att), mutate="one_too_many"), want)
    assert not (neigh == so.SPILL_MARK).any()


def gate_mul_neighbour(P):
    g = _g(10, P)
    return mix_weights(g, P, 4, bias_amp=9)


def test_the_large_case_takes_a_second_trip_everywhere():
    for op, items in large_items(*LARGE).items():
        assert items > ONE_TRIP, (op, items)
