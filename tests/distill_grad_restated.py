"""The gradient of the distillation losses with respect to the student's output, restated in numpy float64 with the
operation order of include/rtpe_hip_distill_grad.h ("Distillation losses: backward").  The
normalisation, the effective mask and the test data are those of tests/distill_restated.py.

``fault=`` switches in one deliberate mistake; tests/test_distill_grad_host.py shows that the stored cases see each.
"""
import numpy as np

import distill_restated as R

f32 = np.float32
FAULTS = ("drop_m", "raw_mask", "sigmoid_raw", "pos_weight", "alpha", "n_channels", "no_upstream", "extra_nonzero",
          "no_factor_2")
GRAD_LOSS = (0.3, -1.5, 2.0)            # an upstream gradient with every entry live and one negative
STORED_SHAPE = (2, 17, 10, 14)          # the fixture holds the reference's gradient itself for this shape ...
STORED_PARAMS = (1, 3)                  # ... and these rows of LOSS_PARAMS


def grad(pred, teacher, gt, alpha, mask, background_factor, kind, pw_t, pw_g, unit=None, grad_loss=(0, 0, 1), fault=None):
    """``(v64, mag)``, both float64 of ``pred``'s shape (N, pred_channels >= J, h, w): the gradient of
    ``g0 teacher_loss + g1 gt_loss + g2 (alpha teacher_loss + (1 - alpha) gt_loss)`` with respect to ``pred`` before its
    one rounding to float32, and the magnitude the error bound is relative to: the sum of the absolute values of the two
    terms whose difference (BCE: ``a s`` and ``b``) or sum (MSE) the gradient is, times ``|m| / n``.  ``teacher`` None:
    its term is absent.  ``unit``: normalise the targets first (default: for "bce").  Channels >= J and elements whose
    effective mask is 0 are +0.0 in both."""
    pred, gt = np.asarray(pred, f32), np.asarray(gt, f32)
    N, J, h, w = gt.shape
    PC = pred.shape[1]
    unit = kind == "bce" if unit is None else unit
    gn, tn, me = R.normalise(gt, teacher, mask, background_factor, unit)
    if fault == "raw_mask" and mask is not None:
        me = np.broadcast_to(np.asarray(mask, f32), gt.shape).copy()
    g0, g1, g2 = (float(f32(g)) for g in grad_loss)
    if fault == "no_upstream":          # a backward that never looks at its argument: every upstream entry taken as 1
        g0 = g1 = g2 = 1.0
    alpha = float(alpha)
    if fault == "alpha":
        alpha = 1.0 - alpha
    wt = g0 + alpha * g2
    wg = g1 + (1.0 - alpha) * g2
    n = float(N * (PC if fault == "n_channels" else J) * h * w)
    p = pred[:, :J]
    if me is not None:
        p, gn = p * me, gn * me
        tn = None if tn is None else tn * me
    x, yg = p.astype(np.float64), gn.astype(np.float64)
    yt = None if tn is None else tn.astype(np.float64)
    md = np.ones(gt.shape) if me is None else me.astype(np.float64)
    if kind == "mse":
        two = 1.0 if fault == "no_factor_2" else 2.0
        tg = (wg * two) * (x - yg)
        tt = np.zeros_like(tg) if yt is None else (wt * two) * (x - yt)
        r = tg if yt is None else tt + tg
        size = np.abs(tt) + np.abs(tg)
    else:
        xs = np.asarray(pred[:, :J], f32).astype(np.float64) if fault == "sigmoid_raw" else x
        e = np.exp(-np.abs(xs))
        d = 1.0 + e
        s = np.where(xs >= 0.0, 1.0 / d, e / d)
        pt, pg = float(f32(pw_t)), float(f32(pw_g))

        def term(wgt, y, pw):
            q = pw * y
            if fault == "pos_weight":           # the weight on the (1 - y) term instead
                return wgt * (pw * (1.0 - y) + y), wgt * y
            return wgt * ((1.0 - y) + q), wgt * q
        a, b = term(wg, yg, pg)
        if yt is not None:
            at, bt = term(wt, yt, pt)
            a, b = at + a, bt + b
        r = (a * s) - b
        size = np.abs(a * s) + np.abs(b)
    v = r / n if fault == "drop_m" else (r * md) / n
    mag = (size * np.abs(md)) / n
    if fault != "drop_m":
        v = np.where(md == 0.0, 0.0, v)
    v64, m64 = np.zeros(pred.shape), np.zeros(pred.shape)
    v64[:, :J], m64[:, :J] = v, mag
    if fault == "extra_nonzero" and PC > J:     # the channel without a target treated like the last one with one
        v64[:, J:] = v[:, J - 1:J]
    return v64, m64


GRAD_UNITS = 10.0


def grad_bound(mag):
    """absolute per-element bound on the distance between the device's float64 gradient (before its rounding to
    float32) and this restatement: ``GRAD_UNITS * 2^-52 * mag``.  Derived the way ``distill_restated.loss_bound`` is, in
    units of 2^-52 (a correctly rounded operation costs half a unit):

    * MSE has no transcendental; every operation is one IEEE operation in the same order on both sides: the distance is
      0 and the device is compared with ``float32(v64)`` bit for bit.  The bound is for BCE.
    * ``x``, ``yt``, ``yg``, ``wt``, ``wg`` are the same float64 numbers on both sides, so ``a`` and ``b``, IEEE
      operations on them in one fixed order, are the same bits on both sides: their roundings move both sides alike and
      cost nothing - which is as well, since with a negative upstream gradient ``a`` and ``b`` cancel and their rounding
      is not small against ``|a|`` or ``|b|``.
    * ``e = exp(-|x|)``: within 1 ulp on the device, within 2 in numpy's vector exp: 3 units between the two.
      ``s = 1 / (1 + e)`` or ``e / (1 + e)`` depends on e with a relative sensitivity of at most 1 (e <= 1): 3 units,
      and the roundings of ``1 + e`` and of the division, half a unit each on each side: 2 more.  5 units of ``|s|``.
    * the product ``a * s`` rounds once on each side: 6 units of ``|a s|``.
    * the difference ``a s - b`` rounds once on each side, half a unit of ``|a s - b| <= |a s| + |b|`` each: 7 units of
      ``|a s| + |b|``.
    * ``* m`` and ``/ n`` round once each on each side: 2 units of the result, which is at most ``mag``: 9 units.
    * the products of these relative errors with each other are below 100 * 2^-104; 1 unit covers them.
    ``mag = (|a s| + |b|) |m| / n``.  Valid while exp neither overflows nor is subnormal: ``|x| < 700``."""
    return GRAD_UNITS * 2.0 ** -52 * np.asarray(mag, np.float64)


def within(got32, v64, mag):
    """the rule of the device test for BCE: got32 lies in the set of float32 roundings of the values within the bound of
    v64 - elementwise ``float32(v64 - b) <= got32 <= float32(v64 + b)``, nothing beyond it.  Returns the boolean array."""
    b = grad_bound(mag)
    return ((v64 - b).astype(f32) <= got32) & (got32 <= (v64 + b).astype(f32))


def case_args(shape, mode, mask_mode, kind, pi):
    """the arguments of ``grad`` for one case of the loss test data"""
    pred, teacher, gt, mask = R.loss_inputs(shape, mode, mask_mode)
    bf, alpha, pw = R.LOSS_PARAMS[pi]
    pw_t, pw_g = R.loss_pos_weights(pw)
    return dict(pred=pred, teacher=teacher, gt=gt, alpha=alpha, mask=mask, background_factor=bf, kind=kind, pw_t=pw_t,
                pw_g=pw_g, unit=kind == "bce")


def all_cases():
    return [(s, m, k, kind, pi) for s in R.LOSS_SHAPES for m in R.LOSS_MODES for k in R.LOSS_MASKS
            for kind in R.LOSS_KINDS for pi in range(len(R.LOSS_PARAMS))]


def stored_cases():
    return [c for c in all_cases() if c[0] == STORED_SHAPE and c[4] in STORED_PARAMS]


def loss_cases():
    return [(s, m, k) for s in R.LOSS_SHAPES for m in R.LOSS_MODES for k in R.LOSS_MASKS]


# ---- shared by the host and the GPU tests: each restated result computed once, handed out read-only ----------------------
_cache = {}


def restated(case, grad_loss=(0, 0, 1)):
    """``grad`` of one case of ``all_cases()``"""
    key = ("grad", case, tuple(grad_loss))
    if key not in _cache:
        v64, mag = grad(grad_loss=grad_loss, **case_args(*case))
        v64.setflags(write=False)
        mag.setflags(write=False)
        _cache[key] = (v64, mag)
    return _cache[key]


def effective_mask(case):
    a = case_args(*case)
    return R.normalise(a["gt"], a["teacher"], a["mask"], a["background_factor"], a["unit"])[2]


def target_maps(i):
    """the restated targets of ``distill_restated.TARGET_CASES[i]``"""
    key = ("targets", i)
    if key not in _cache:
        image_hw, det_hw, att_hw, _ = R.TARGET_CASES[i]
        people, teacher, mask, segm = R.target_inputs(R.TARGET_CASES[i])
        _cache[key] = R.targets(people, R.TARGET_J, image_hw, det_hw, att_hw, teacher, mask, segm)
    return _cache[key]


def crossed(got32, want32, v64):
    """for elements where the float32 ``got32`` differs from ``want32 = float32(v64)``: the distance from ``v64`` to the
    nearest value that rounds to ``got32`` - the rounding boundary on got32's side, the midpoint of got32 and its
    float32 neighbour towards v64 (for adjacent values that is the midpoint of the two).  0 where they agree."""
    got32, want32 = np.asarray(got32, f32), np.asarray(want32, f32)
    toward = np.nextafter(got32, want32)
    edge = (got32.astype(np.float64) + toward.astype(np.float64)) / 2
    return np.where(got32 != want32, np.abs(edge - v64), 0.0)


def grad_key(shape, mode, mask_mode, kind, pi):
    return "grad/" + R.loss_key(shape, mode, mask_mode, kind, pi)[len("loss/"):]
