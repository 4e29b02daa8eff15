"""The students' eight small fp32 ops (csrc/student_ops.hip) in float64 with the kernels' rounding points.

Companion of oracle/exact.py: one function per op on NCHW float64 tensors that hold fp32 values, each returning THE
fp32 answer (held in float64).  On the data the tests use - integers well below 2^24, weights in {-1, 0, 1} - every sum
is exact in any order, so each fp32 operation of a kernel is one round-to-nearest of an exactly known number and
``_f32`` (one rounding of the float64 value) restates it.  A float64 quotient or product of two fp32 numbers rounded
once more to fp32 is the correctly rounded fp32 result (53 >= 2 * 24 + 2 bits).

The sigmoid is the one place without a single right bit pattern, because ``expf`` on the device is not correctly
rounded.  It is judged in two ways (``sigmoid_check``):

  exact points    argument == 0 gives 0.5; argument >= 18 gives 1.0 (1 + e^-18 rounds to 1); argument <= -104 gives 0.0
                  (``expf`` overflows to infinity).  Arguments in (-104, -80) are kept out of the data: there fp32 and
                  float64 disagree by design (denormal results).
  generic band    |argument| <= 80, against the float64 sigmoid, within ``4 + |argument|`` ulps of the fp32 result:
                  the division ``l / div`` leaves the argument with a relative error of 2^-24, which e^-a turns into up
                  to |a| ulps of the result; 1 ulp for ``expf`` (the bound of the HIP math API reference, table of the
                  single precision functions: ``expf`` 1 ulp), half an ulp each for the add and the divide, and one for
                  ulp boundaries (the result may sit just below a power of two, where the ulp halves).

``mutate=`` names one seeded fault per op (``MUTATIONS``): what a kernel with that fault would give.
tests/test_student_ops_host.py shows that the data of every GPU case sees the faults that apply to it."""
import types

import numpy as np
import torch
import torch.nn.functional as F

MUTATIONS = {
    "avgpool": ("div9", "shifted"),
    "se_gate": ("mean_short", "no_b1", "no_relu", "last_gate_zero"),
    "cam_combine": ("gate_of_image0", "no_relu"),
    "sigmoid_map": ("div_ignored", "div20_unasked"),
    "resize": ("no_clamp0", "no_clamps", "align_corners", "swapped_weights"),
    "aux_pack": ("pad_nonzero", "swap_rb"),
    "place": ("one_too_many",),
}
SIG_ONE, SIG_ZERO, SIG_BAND = 18.0, -104.0, 80.0
SPILL_MARK = 7777.0            # what a store one channel too far leaves there (any value the neighbour does not hold)


def _f32(v):
    """one round-to-nearest of float64 values to fp32"""
    return v.float().double()


def is_f32(v):
    return bool(torch.equal(v.float().double(), v))


def _mut(op, mutate):
    assert mutate is None or mutate in MUTATIONS[op], (op, mutate)
    return mutate


def exact_conv(x, w, bias=None, stride=1, relu=False, quantum=1.0):
    """an fp32 conv layer (alpha = 1, beta = bias) on data whose sums are exact in any order: x a multiple of
    ``quantum``, w in {-1, 0, 1}, bias a multiple of the quantum, taps * max|x| / quantum + max|bias| below 2^24 (the
    bound of the conv tests' ``_ref_layer``)"""
    k = w.shape[-1]
    taps = w.shape[1] * k * k
    assert torch.equal(torch.round(x / quantum) * quantum, x), "x is not a multiple of the quantum"
    assert torch.equal(torch.round(w), w) and float(w.abs().max()) <= 1
    top = taps * float(x.abs().max()) / quantum + (float(bias.abs().max()) / quantum if bias is not None else 0.0)
    assert top < 2 ** 24, "sums are not exact in fp32: %g quanta" % top
    y = F.conv2d(x, w, bias, stride, k // 2)
    assert is_f32(y)
    return torch.where(y > 0, y, torch.zeros_like(y)) if relu else y


def cast(x):
    """fp16 -> fp32: exact"""
    assert torch.equal(x.half().double(), x), "not fp16 values"
    return x


def avgpool(x, mutate=None):
    """AvgPool2d(3, 2, 1, count_include_pad=False): the exact sum of the taps inside, divided by their number"""
    m = _mut("avgpool", mutate)
    assert torch.equal(torch.round(x * 8) / 8, x) and 9 * float(x.abs().max()) * 8 < 2 ** 24, "the window sum is not exact"
    ones = torch.ones((1, 1) + tuple(x.shape[2:]), dtype=torch.float64)
    if m == "shifted":                                  # the window starts at 2 * o instead of 2 * o - 1
        Ho, Wo = (x.shape[2] + 1) // 2, (x.shape[3] + 1) // 2
        pad = (0, 2 * Wo + 1 - x.shape[3], 0, 2 * Ho + 1 - x.shape[2])
        s = F.avg_pool2d(F.pad(x, pad), 3, 2, 0, divisor_override=1)
        cnt = F.avg_pool2d(F.pad(ones, pad), 3, 2, 0, divisor_override=1)
    else:
        s = F.avg_pool2d(x, 3, 2, 1, divisor_override=1)
        cnt = F.avg_pool2d(ones, 3, 2, 1, divisor_override=1)
    out = _f32(s / (9.0 if m == "div9" else cnt))
    return types.SimpleNamespace(out=out, counts=sorted(set(int(c) for c in cnt.flatten().tolist())))


def sigmoid64(a):
    return 1.0 / (1.0 + torch.exp(-a))


def se_gate(x, w1, b1, w2, b2, mutate=None):
    """SELayer: sigmoid(W2 relu(W1 mean_hw(x) + b1) + b2) per image.  The means, both layers and the logits must be
    integers (asserted): only the sigmoid is then inexact.  Returns the logits (N, C) and ``gate``, the float64 sigmoid
    with the exact points put in (``sigmoid_check`` judges a kernel's gate against the logits)."""
    m = _mut("se_gate", mutate)
    N, C, H, W = x.shape
    HW = H * W
    flat = x.flatten(2)
    if m == "mean_short" and HW > 1:                    # the pixel loop ends one early
        mean = flat[..., :-1].sum(-1) / (HW - 1)
    else:
        assert float(flat.abs().sum(-1).max()) < 2 ** 24, "the pixel sum is not exact"
        mean = flat.sum(-1) / HW
        assert torch.equal(torch.round(mean), mean), "a channel mean is not an integer"
    h = mean @ w1.t() + (0 if m == "no_b1" else b1)
    if m != "no_relu":
        h = torch.where(h > 0, h, torch.zeros_like(h))
    logit = h @ w2.t() + b2
    if m is None:
        assert torch.equal(torch.round(logit), logit) and float(logit.abs().max()) < 2 ** 24
        assert float(h.abs().sum(-1).max()) + float(b2.abs().max()) < 2 ** 24
    gate = sigmoid_map(logit).want
    if m == "last_gate_zero":
        gate = gate.clone()
        gate[:, -1] = 0
    return types.SimpleNamespace(logit=logit, gate=gate, mean=mean)


def cam_combine(res, hdc, gate, mutate=None):
    """relu(res + hdc * gate[n, c]) with the product and the sum rounded separately (the build contracts nothing);
    ``gate`` (N, C) holds fp32 values"""
    m = _mut("cam_combine", mutate)
    assert is_f32(gate) and is_f32(res) and is_f32(hdc)
    g = gate[:1].expand_as(gate) if m == "gate_of_image0" else gate
    out = _f32(res + _f32(hdc * g[:, :, None, None]))
    return out if m == "no_relu" else torch.where(out > 0, out, torch.zeros_like(out))


def sigmoid_arg(l, div=None, mutate=None):
    m = _mut("sigmoid_map", mutate)
    if m == "div_ignored":
        div = None
    if m == "div20_unasked" and div is None:
        div = 20.0
    return l / div if div else l


def sigmoid_map(l, div=None, mutate=None):
    """sigmoid(l / div) (``div`` None: no division).  ``arg`` is the exact quotient, ``want`` the float64 sigmoid with
    the three exact points put in, ``exact`` the mask of the elements that have one right fp32 bit pattern."""
    a = sigmoid_arg(l, div, mutate)
    exact = (a == 0) | (a >= SIG_ONE) | (a <= SIG_ZERO)
    want = torch.where(a >= SIG_ONE, torch.ones_like(a), torch.where(a <= SIG_ZERO, torch.zeros_like(a), sigmoid64(a)))
    return types.SimpleNamespace(arg=a, want=want, exact=exact)


def sigmoid_check(got, l, div=None):
    """judges fp32 values ``got`` against sigmoid(l / div): ``array_equal`` at the exact points, ``4 + |argument|`` ulps
    of the fp32 result in the generic band.  Returns (ok, largest error in ulps, its argument, largest share of the
    budget, number of wrong exact points)."""
    s = sigmoid_map(l, div)
    a = s.arg
    assert not (((a > SIG_ZERO) & (a < -SIG_BAND)) | ((a > SIG_BAND) & (a < SIG_ONE))).any(), "an argument outside the bands"
    got = got.double()
    wrong_exact = int(((got != s.want) & s.exact).sum())
    band = ~s.exact
    if not band.any():
        return wrong_exact == 0, 0.0, 0.0, 0.0, wrong_exact
    w = s.want[band]
    ulp = torch.from_numpy(np.spacing(w.float().numpy()).astype(np.float64))
    err = (got[band] - w).abs() / ulp
    budget = 4.0 + a[band].abs()
    share = err / budget
    i = int(err.argmax())
    ok = wrong_exact == 0 and bool((share <= 1.0).all()) and bool(torch.isfinite(got).all())
    return ok, float(err[i]), float(a[band][i]), float(share.max()), wrong_exact


def sigmoid_add(x, att):
    """x + att (att (N, 1, H, W) broadcast over the channels): one rounding"""
    assert is_f32(x) and is_f32(att)
    return _f32(x + att)


def gate_mul(x, att):
    assert is_f32(x) and is_f32(att)
    return _f32(x * att)


def aux_pack(aux, mutate=None):
    """(N, 3, H, W) -> the four channels r, g, b, +0: a copy"""
    m = _mut("aux_pack", mutate)
    a = aux[:, [2, 1, 0]] if m == "swap_rb" else aux
    pad = torch.full_like(aux[:, :1], 1.0 if m == "pad_nonzero" else 0.0)
    return torch.cat([a, pad], 1)


def _axis(n_in, n_out, mutate):
    """indices and weights of one axis of PyTorch-CPU's half-pixel bilinear, each fp32 operation rounded once"""
    o = torch.arange(n_out, dtype=torch.float64)
    if n_in == n_out and mutate != "align_corners":
        i = torch.arange(n_out)
        return types.SimpleNamespace(i0=i, i1=i, l0=torch.ones(n_out, dtype=torch.float64),
                                     l1=torch.zeros(n_out, dtype=torch.float64), clamp0=False, edge=False, shortcut=True)
    if mutate == "align_corners":
        scale = _f32(torch.tensor((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0, dtype=torch.float64))
        real = _f32(scale * o)
    else:
        scale = _f32(torch.tensor(float(n_in), dtype=torch.float64) / float(n_out))
        real = _f32(scale * (o + 0.5) - 0.5)            # one fma: the float64 expression is exact (24 + 12 bits)
    clamp0 = bool((real < 0).any())
    if mutate not in ("no_clamp0", "no_clamps"):
        real = torch.clamp(real, min=0.0)
    a = torch.clamp(torch.trunc(real), max=n_in - 1)
    edge = bool((a == n_in - 1).any())
    i0 = a.long()
    i1 = i0 + (i0 < n_in - 1).long()
    lam = _f32(real - a)
    if mutate != "no_clamps":
        lam = torch.clamp(lam, 0.0, 1.0)
    return types.SimpleNamespace(i0=i0, i1=i1, l0=_f32(1.0 - lam), l1=lam, clamp0=clamp0, edge=edge, shortcut=False)


def resize(x, Ho, Wo, mutate=None):
    """F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=False) as PyTorch-CPU's fp32 kernel computes it:
    real = fma(scale, o + 0.5, -0.5) clamped at 0, lambda clamped to [0, 1], t = fma(v0, l0, v1 * l1) along x, the same
    along y.  ``info`` says whether the clamp at 0 and the last-row / last-column edge act on each axis."""
    m = _mut("resize", mutate)
    assert is_f32(x)
    N, C, Hi, Wi = x.shape
    am = m if m in ("no_clamp0", "no_clamps", "align_corners") else None
    ay, ax = _axis(Hi, Ho, am), _axis(Wi, Wo, am)
    wy0, wy1, wx0, wx1 = ay.l0, ay.l1, ax.l0, ax.l1
    if m == "swapped_weights":                          # the x weights used along y and the y weights along x
        pick = lambda v, k: v[torch.arange(k) % v.numel()]
        wy0, wy1, wx0, wx1 = pick(ax.l0, Ho), pick(ax.l1, Ho), pick(ay.l0, Wo), pick(ay.l1, Wo)
    rows0, rows1 = x[:, :, ay.i0], x[:, :, ay.i1]
    lx0, lx1 = wx0.view(1, 1, 1, -1), wx1.view(1, 1, 1, -1)
    t0 = _f32(rows0[..., ax.i0] * lx0 + _f32(rows0[..., ax.i1] * lx1))
    t1 = _f32(rows1[..., ax.i0] * lx0 + _f32(rows1[..., ax.i1] * lx1))
    out = _f32(t0 * wy0.view(1, 1, -1, 1) + _f32(t1 * wy1.view(1, 1, -1, 1)))
    return types.SimpleNamespace(out=out, y=ay, x=ax)


def place(dst, coff, val, mutate=None):
    """an op's store into channels [coff, coff + C) of the NHWC rows of ``dst`` (N, ld, H, W); returns the new tensor.
    ``one_too_many``: the store runs one channel on - into the neighbour's first channel, or, from the last channel of
    a row, into the next pixel's first (the very last pixel's falls outside the tensor and is left to the guards)"""
    m = _mut("place", mutate)
    C = val.shape[1]
    out = dst.clone()
    out[:, coff:coff + C] = val
    if m == "one_too_many":
        ld = dst.shape[1]
        rows = out.permute(0, 2, 3, 1).reshape(-1)
        idx = torch.arange(dst.shape[0] * dst.shape[2] * dst.shape[3]) * ld + coff + C
        rows[idx[idx < rows.numel()]] = SPILL_MARK
        out = rows.view(dst.shape[0], dst.shape[2], dst.shape[3], ld).permute(0, 3, 1, 2).contiguous()
    return out


# --------------------------------------------------------------------------- #
# seeded data
# --------------------------------------------------------------------------- #
def logits_for(div, count, seed):
    """``count`` integer logits for sigmoid(l / div): the three exact points, their neighbours inside the bands, the ends
    of the generic band, and random integers of the band |l / div| <= 80"""
    d = float(div) if div else 1.0
    up, lo, band = int(np.ceil(SIG_ONE * d)), int(np.floor(SIG_ZERO * d)), int(np.floor(SIG_BAND * d))
    fixed = [0, 1, -1, up, up + 1, 4 * up, 1000 * up, lo, lo - 1, 4 * lo, 1000 * lo, band, -band, band - 1, 1 - band]
    g = torch.Generator().manual_seed(seed)
    assert count > len(fixed)
    rnd = torch.randint(-band, band + 1, (count - len(fixed),), generator=g)
    l = torch.cat([torch.tensor(fixed), rnd]).double()
    return l[torch.randperm(count, generator=g)]


def zero_sum_pattern(H, W, channels, g, amp=3):
    """(channels, H, W) integers whose sum over the map is zero per channel (f(y, x) - f(H-1-y, W-1-x)): added to a
    per-image, per-channel constant it leaves the mean that constant"""
    f = torch.randint(-amp, amp + 1, (channels, H, W), generator=g).double()
    p = f - f.flip(1, 2)
    if H * W > 1:
        p[:, -1, -1] = torch.where(p[:, -1, -1] == 0, torch.ones(channels, dtype=torch.float64), p[:, -1, -1])
        p[:, 0, 0] = -p[:, -1, -1]                      # the last pixel never holds a zero (a loop that ends early shows)
    assert torch.equal(p.sum((1, 2)), torch.zeros(channels, dtype=torch.float64))
    return p
