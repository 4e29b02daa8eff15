"""The order-independent conv data of oracle/exact.py, checked on the CPU.

(1) Order independence: on this data PyTorch-CPU's fp32 convolution gives the float64 result bit for bit with oneDNN
    on, with oneDNN off and with the input channels permuted - three accumulation orders nobody controls - and the
    BatchNorm value is an fp32 number.  So the expected output of tests/test_conv_exact_gpu.py is THE answer for any
    kernel that accumulates in fp32, not one implementation's.
(2) The data can see faults: each seeded fault of ``exact.MUTATIONS``, applied to the reference, changes at least one
    output element in every (class, regime) where it applies.  Where a fault cannot apply it is not silently passed:
    ``applies`` states the rule, and the test asserts that the fault is indeed invisible there only because the data
    holds nothing for it to act on.

The case tables of the GPU file live here, so that both files walk the same list."""
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
