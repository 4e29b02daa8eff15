"""Inputs for which a convolution layer has ONE right answer, bit for bit, whatever the accumulation order.

Every input and weight is an integer multiple of one power of two (the *quantum* of the case) and
(number of taps) x max|x| x max|w| stays below 2^24 quanta.  Then every product and every partial sum of the
convolution, taken in any order and on any pipe, is exactly representable in fp32: fp32 accumulation is exact,
and the float64 convolution is the result itself, not an approximation of it.  Each later rounding of the half
wrapper (include/rtpe_hip.h: ``y = act(round16(round16?(conv) * alpha + beta) [+ res])``) is then
round-to-nearest of an exactly known number, so a kernel is compared with ``array_equal`` - no tolerance and
no share of elements left out.  tests/test_conv_exact_host.py shows that PyTorch-CPU's fp32 convolution agrees
with the float64 one on this data under three different accumulation orders, and that the data can see the
faults a kernel may have; tests/test_conv_exact_gpu.py runs the HIP kernels on it.

Regimes (``w`` is always drawn from {-1, 0, 1} times a power of two):

  ``int``      x integers in [-3, 3]; alpha in {0.5, 0.75, ..., 1.5}, beta a multiple of 1/4 in [-8, 8]:
               indexing, taps, borders, channel padding (the conv rounding is the identity);
  ``denorm``   x = k * 2^-24, |k| <= 1023 (every input an fp16 denormal or zero), w * 2^6, beta * 2^-8:
               normal-range outputs that mostly are NOT fp16 values, so every rounding point is exercised and
               a flush of fp16 denormals anywhere moves them;
  ``cancel``   x = +-(1024 + j), j in [0, 7], random signs, w * 2^-6: terms that cancel to results far
               below the sum of their magnitudes; outputs stay finite;
  ``overflow`` ``int`` data with alpha and beta so large that part of the BatchNorm output exceeds 65504:
               the expected output holds +-inf where the half wrapper's does, and never a NaN (the residual
               is finite).

With ``f32=True`` everything is integer-valued and stays below 2^24 through BatchNorm and the add: no
rounding happens anywhere and the fp32 kernels must be bit-exact as well.
"""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

REGIMES = ("int", "denorm", "cancel", "overflow")
IN_SENTINEL = 30000.0          # finite in fp16: garbage * zero weight stays harmless, garbage that reaches a sum does not
OUT_PATTERN = {2: 0x7D5A, 4: 0x7FC5A5A5}     # NaN payloads no kernel result can carry
MUTATIONS = ("drop_tap", "halo_sentinel", "flush_denormals", "conv_rtz", "conv_unrounded", "single_rounding",
             "skip_last_chunk")
_W_SCALE = {"int": 1.0, "denorm": 2.0 ** 6, "cancel": 2.0 ** -6, "overflow": 1.0}
_X_QUANTUM = {"int": 1.0, "denorm": 2.0 ** -24, "cancel": 1.0, "overflow": 1.0}


def _is_f32(v):
    """every element of the float64 tensor is an fp32 value (or the tensor holds what .float() keeps)"""
    return bool(torch.equal(v.float().double(), v))


def round16(v):
    """round-to-nearest-even of exactly known fp32 values (held in float64) to fp16; beyond 65504 + half a step: +-inf"""
    assert _is_f32(v), "the value to round is not an fp32 number: the kernel's own fp32 step would round first"
    return v.float().half().double()


def round16_toward_zero(v):
    h = v.float().half()
    hn = h.numpy()
    away = np.abs(hn.astype(np.float64)) > np.abs(v.numpy())
    hn = np.where(away, np.nextafter(hn, np.float16(0)), hn)
    return torch.from_numpy(hn.astype(np.float64))


def _draw_x(regime, shape, g):
    if regime in ("int", "overflow"):
        return torch.randint(-3, 4, shape, generator=g).double()
    if regime == "denorm":
        return torch.randint(-1023, 1024, shape, generator=g).double() * 2.0 ** -24
    if regime == "cancel":
        sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
        return sign * (1024 + torch.randint(0, 8, shape, generator=g)).double()
    raise ValueError(regime)


def _draw_res(regime, shape, g, f32):
    if f32:
        return torch.randint(-8, 9, shape, generator=g).double()
    if regime in ("int", "overflow"):
        return torch.randint(-128, 129, shape, generator=g).double() / 16
    if regime == "denorm":
        return torch.randint(-1023, 1024, shape, generator=g).double() * 2.0 ** -13
    return torch.randint(-256, 257, shape, generator=g).double() / 4


def _draw_affine(regime, cout, taps, g, f32):
    if f32:
        return torch.randint(1, 4, (cout,), generator=g).double(), torch.randint(-8, 9, (cout,), generator=g).double()
    alpha = torch.randint(2, 7, (cout,), generator=g).double() / 4
    beta = torch.randint(-32, 33, (cout,), generator=g).double() / 4
    if regime == "denorm":
        beta = beta * 2.0 ** -8
    if regime == "overflow":
        # the conv of `int` data has a standard deviation of sqrt(taps * 2/3 * 4): scale alpha by the power of two
        # that puts one standard deviation next to the largest fp16 number, beta to a few thousand
        sd = math.sqrt(taps * 8.0 / 3.0)
        alpha = alpha * 2.0 ** round(math.log2(65504.0 / sd))
        beta = beta * 1024
    return alpha, beta


def _conv64(x, w, k, stride, dilation, transposed):
    if transposed:
        return F.conv_transpose2d(x, w, None, 2, 1)
    return F.conv2d(x, w, None, stride, dilation * (k // 2), dilation)


@functools.lru_cache(maxsize=4)
def _base(cin, cout, k, stride, dilation, N, H, W, regime, seed, f32, transposed):
    """x, w and the float64 convolution of a case: shared by every flag combination of it"""
    assert regime in REGIMES and (not f32 or regime == "int")
    g = torch.Generator().manual_seed(seed)
    x = _draw_x(regime, (N, cin, H, W), g)
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    w = torch.randint(-1, 2, wshape, generator=g).double() * _W_SCALE[regime]
    taps = cin * (4 if transposed else k * k)         # a transposed k4 s2 conv gathers 2 x 2 taps per output
    quantum = _X_QUANTUM[regime] * _W_SCALE[regime]
    # the preconditions of order independence
    assert torch.equal(x.half().double(), x) and torch.equal(w.half().double(), w), "x, w must be fp16 values"
    assert taps * float(x.abs().max()) * float(w.abs().max()) / quantum < 2 ** 24
    conv = _conv64(x, w, k, stride, dilation, transposed)
    assert _is_f32(conv) and torch.equal(torch.round(conv / quantum) * quantum, conv)
    alpha, beta = _draw_affine(regime, cout, taps, g, f32)
    res = _draw_res(regime, tuple(conv.shape), g, f32)
    return x, w, conv, alpha, beta, res, quantum


def reference(x, w, alpha, beta, res, k, stride, dilation, relu, round_conv, f32=False, transposed=False, conv=None,
              mutate=None):
    """The layer in float64 with the half wrapper's rounding points; returns every intermediate.

    ``mutate`` names one seeded fault (MUTATIONS): what a kernel with that fault would give.  The tests apply them
    to show that the data of a case can see the fault."""
    assert mutate is None or mutate in MUTATIONS
    if mutate == "flush_denormals":                     # fp16 denormal inputs read as zero
        x = torch.where(x.abs() < 2.0 ** -14, torch.zeros_like(x), x)
        conv = None
    if mutate == "skip_last_chunk":                     # the last 16 input channels (one MFMA k step) never accumulated
        x = x.clone()
        x[:, -16:] = 0
        conv = None
    if mutate == "halo_sentinel":                       # the halo row below the image holds the guard value, not zero
        assert not transposed
        pad = dilation * (k // 2)
        xp = F.pad(x, (pad, pad, pad, pad))
        xp[:, :, pad + x.shape[2]:, pad:pad + x.shape[3]] = IN_SENTINEL
        conv = F.conv2d(xp, w, None, stride, 0, dilation)
    if conv is None:
        conv = _conv64(x, w, k, stride, dilation, transposed)
    if mutate == "drop_tap":                            # the centre tap of the last output channel at the last column
        assert not transposed
        conv = conv.clone()
        c = k // 2
        conv[:, -1, :, -1] -= torch.einsum("nih,i->nh", x[:, :, ::stride, (conv.shape[3] - 1) * stride][:, :, :conv.shape[2]],
                                           w[-1, :, c, c])
    a, b = alpha.view(1, -1, 1, 1), beta.view(1, -1, 1, 1)
    # (a mutated value need not be an fp32 number: round it as it is)
    r16 = (lambda v: v) if f32 else round16 if mutate is None else (lambda v: v.float().half().double())
    if f32 or not round_conv or mutate == "conv_unrounded":
        conv_r = conv
    elif mutate == "conv_rtz":
        conv_r = round16_toward_zero(conv)
    else:
        conv_r = r16(conv)
    bn = conv_r * a + b                                  # exact in float64: <= 24 + 3 + a few bits
    if mutate is None:
        assert _is_f32(bn), "the BatchNorm value must be an fp32 number (the kernel's fmaf then rounds nothing)"
    if mutate == "single_rounding" and res is not None:
        out = r16(bn + res)
    else:
        bn_r = r16(bn)
        out = r16(bn_r + res) if res is not None else bn_r
    if relu:                                            # the kernels' `v > 0 ? v : 0`: +0 for -0, for -inf (and for a NaN)
        out = torch.where(out > 0, out, torch.zeros_like(out))
    return types.SimpleNamespace(conv=conv, conv_r=conv_r, bn=bn, out=out)


def exact_case(cin, cout, k, stride, dilation, N, H, W, regime, seed, residual, relu, round_conv, f32=False,
               transposed=False, mutate=None):
    """One seeded layer case: x (N, cin, H, W), w (OIHW; IOHW when transposed), alpha, beta, res (or None) as the
    kernel's dtypes (fp16 / fp32 tensors, alpha and beta fp32), and ``want``, the expected output in that dtype
    (NCHW); ``ref`` holds the float64 intermediates.  ``H, W`` are the INPUT size."""
    x, w, conv, alpha, beta, res, quantum = _base(cin, cout, k, stride, dilation, N, H, W, regime, seed, bool(f32),
                                                   bool(transposed))
    r = reference(x, w, alpha, beta, res if residual else None, k, stride, dilation, relu, round_conv, f32, transposed,
                  conv=conv, mutate=mutate)
    dt = torch.float32 if f32 else torch.float16
    assert not torch.isnan(r.out).any()
    assert f32 is False or float(r.out.abs().max()) < 2 ** 24
    return types.SimpleNamespace(x=x.to(dt), w=w.to(dt), alpha=alpha.float(), beta=beta.float(),
                                 res=res.to(dt) if residual else None, want=r.out.to(dt), ref=r, quantum=quantum,
                                 x64=x, w64=w, alpha64=alpha, beta64=beta, res64=res if residual else None)


def exact_block(N, H, W, seed):
    """A BasicBlock of a 48-channel branch on `int` data: y = relu(bn2(conv(relu(bn1(conv(x))))) + x), both layers with
    the conv's own rounding.  The first layer's output stays below 512, so its fp16 values are exact multiples of 1/4
    and the second conv's sums (432 taps x 512 x 4 quanta < 2^24) stay exact."""
    c1 = exact_case(48, 48, 3, 1, 1, N, H, W, "int", seed, False, True, True)
    mid = c1.ref.out
    g = torch.Generator().manual_seed(seed + 7919)
    w2 = torch.randint(-1, 2, (48, 48, 3, 3), generator=g).double()
    alpha2, beta2 = _draw_affine("int", 48, 432, g, False)
    assert float(mid.abs().max()) < 512 and torch.equal(torch.round(mid * 4) / 4, mid)
    r2 = reference(mid, w2, alpha2, beta2, c1.x64, 3, 1, 1, True, True)
    return types.SimpleNamespace(x=c1.x, w1=c1.w, alpha1=c1.alpha, beta1=c1.beta, w2=w2.half(), alpha2=alpha2.float(),
                                 beta2=beta2.float(), mid=mid.half(), want=r2.out.half(), ref1=c1.ref, ref2=r2)


# --------------------------------------------------------------------------- #
# guard bands
# --------------------------------------------------------------------------- #
def guarded(t, sentinel, device="cuda:0"):
    """A device copy of ``t`` in the middle of a larger allocation: one guard band before it and one after it, each
    at least a full tile row of pixels (34 halo pixels of the widest tile, and never under 64 KiB), the tensor itself
    256-byte aligned.  ``sentinel`` is a float (input guards: a finite value, IN_SENTINEL) or an int (output guards:
    a bit pattern, OUT_PATTERN[itemsize]; the tensor's own elements are then preset to it too, so an element the
    kernel never writes shows up in the comparison)."""
    es = t.element_size()
    assert es in (2, 4)
    guard_bytes = max(65536, (34 * t.shape[-1] * es + 255) // 256 * 256)
    ge, n = guard_bytes // es, t.numel()
    idt = torch.int16 if es == 2 else torch.int32
    buf = torch.empty(2 * ge + (n * es + 255) // 256 * 256 // es, dtype=idt, device=device)
    if isinstance(sentinel, float):
        assert math.isfinite(sentinel)
        bits = int(torch.tensor([sentinel], dtype=t.dtype).view(idt)[0])
        buf.fill_(bits)
        buf[ge:ge + n].copy_(t.contiguous().view(idt).reshape(-1))
    else:
        bits = sentinel - (1 << (8 * es)) if sentinel >= 1 << (8 * es - 1) else sentinel
        buf.fill_(bits)
    view = buf[ge:ge + n].view(t.dtype).view(t.shape)
    assert view.data_ptr() % 256 == 0
    return types.SimpleNamespace(buf=buf, t=view, lo=ge, hi=ge + n, bits=bits)


def guarded_out(shape, dtype, device="cuda:0"):
    return guarded(torch.empty(shape, dtype=dtype), OUT_PATTERN[torch.empty((), dtype=dtype).element_size()], device)


def guards_intact(*gs):
    """True when both guard bands (and the alignment padding) of every guarded tensor still hold their fill"""
    ok = True
    for i, g in enumerate(gs):
        if g is None:
            continue
        for name, part, off in (("before", g.buf[:g.lo], 0), ("after", g.buf[g.hi:], g.hi)):
            bad = torch.nonzero(part != g.bits).flatten()
            if bad.numel():
                ok = False
                print("guard band %s tensor %d overwritten at %d elements; first at element offset %d (tensor spans "
                      "[%d, %d))" % (name, i, bad.numel(), int(bad[0]) + off, g.lo, g.hi))
    return ok


def first_differences(got, want, limit=8):
    """text for an assertion message: the first differing indices of two arrays with got and want"""
    gi = got.view(np.int16 if got.itemsize == 2 else np.int32)
    wi = want.view(np.int16 if want.itemsize == 2 else np.int32)
    bad = np.argwhere(gi != wi)
    rows = ["%s got %r want %r" % (tuple(int(v) for v in ix), got[tuple(ix)], want[tuple(ix)]) for ix in bad[:limit]]
    return "%d of %d elements differ; first: %s" % (len(bad), got.size, "; ".join(rows))
