"""numpy / torch-CPU restatement of the heatmap -> keypoint decode (oracle).

Test infrastructure (see oracle/__init__.py).  Follows
/root/reference/rtpe/third_party/group.py (``HeatmapParser`` :125-287,
``match_by_tag`` :26-97, ``Params`` :100-110) and the two bilinear upsamples
of /root/reference/validate_hhrnet.py:94-98.  Written to make every rounding
and ordering decision explicit, because the HIP kernels and the C++ host
matcher have to reproduce them bit for bit:

* bilinear, align_corners=True, fp32, *as PyTorch-CPU evaluates it*:
  ``T = fma(v0, lx0, v1*lx1)`` per row, ``out = fma(T0, ly0, T1*ly1)``,
  ``l1 = clamp(scale*dst - i0, 0, 1)``, ``l0 = 1 - l1``,
  ``scale = float32(in-1) / float32(out-1)`` (found by experiment against
  ``F.interpolate`` in the build container, see ``bilinear_explicit``).
* numpy float32 means: 8-way pairwise over a contiguous 1-D run
  (``np.mean`` of (n,1) tags, ``ans[:,2].mean()``), plain sequential when the
  reduced axis is not the only one (D > 1 tags).
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from .hungarian_ref import munkres_compute

f32 = np.float32


class Params:
    """group.py:100-110 (joint_order is the identity, :110)"""

    def __init__(self, num_joints=17, max_num_people=30, detection_threshold=0.1,
                 tag_threshold=1.0, use_detection_val=True, ignore_too_much=False):
        self.num_joints = num_joints
        self.max_num_people = max_num_people
        self.detection_threshold = detection_threshold
        self.tag_threshold = tag_threshold
        self.use_detection_val = use_detection_val
        self.ignore_too_much = ignore_too_much


# --------------------------------------------------------------------------- #
# bilinear upsample (validate_hhrnet.py:94-98)
# --------------------------------------------------------------------------- #
def upsample_bilinear(x, h, w):
    """the stock op the reference calls"""
    return F.interpolate(x, (h, w), mode="bilinear", align_corners=True)


def _fma32(a, b, c):
    # exact product and sum in f64 (24+24 bit products are exact; the sum of an
    # exact product and an f32 rounds once when cast back) == fused multiply-add
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def bilinear_axis(n_in, n_out):
    """source indices and weights of one axis (align_corners=True)"""
    if n_in == n_out:
        i0 = np.arange(n_out)
        return i0, i0.copy(), np.ones(n_out, f32), np.zeros(n_out, f32)
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    real = scale * np.arange(n_out).astype(f32)
    i0 = np.minimum(real.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(real - i0.astype(f32), 0, 1).astype(f32)
    return i0, i1, (f32(1) - l1).astype(f32), l1


def bilinear_explicit(x, h, w):
    """explicit formula, bit-equal to ``upsample_bilinear`` on the CPU
    (tests/test_oracle_golden.py::test_bilinear_formula)"""
    x = np.asarray(x, f32)
    y0, y1, ly0, ly1 = bilinear_axis(x.shape[-2], h)
    x0, x1, lx0, lx1 = bilinear_axis(x.shape[-1], w)
    r0, r1 = x[..., y0, :], x[..., y1, :]
    t0 = _fma32(r0[..., x0], lx0, r0[..., x1] * lx1)
    t1 = _fma32(r1[..., x0], lx0, r1[..., x1] * lx1)
    return _fma32(t0, ly0[:, None], t1 * ly1[:, None])


# --------------------------------------------------------------------------- #
# numpy reduction orders
# --------------------------------------------------------------------------- #
def pairwise8_sum_f32(a):
    """numpy's contiguous float32 add.reduce for n <= 128"""
    a = np.asarray(a, f32)
    n = a.shape[0]
    if n < 8:
        s = f32(0)
        for v in a:
            s = f32(s + v)
        return s
    r = [f32(a[i]) for i in range(8)]
    i = 8
    while i + 8 <= n:
        for j in range(8):
            r[j] = f32(r[j] + a[i + j])
        i += 8
    s = f32(f32(f32(r[0] + r[1]) + f32(r[2] + r[3])) + f32(f32(r[4] + r[5]) + f32(r[6] + r[7])))
    while i < n:
        s = f32(s + a[i])
        i += 1
    return s


# Deliberately WRONG float orders (and other seeded faults) that ``refine`` / ``match_by_tag`` can be asked for: the
# scenes of oracle/tagdims.py are built so that each one changes a result (tests/test_decode_dims_host.py).
#   sequential     sum of squares left to right also for D >= 8 (refine; the float64 distances of the matcher)
#   float64        refine's squares accumulated in float64
#   fma            refine's squares contracted into the running sums (one rounding per step)
#   no_tail        the elements behind the last full block of 8 dropped (D = 9, 17)
#   pairwise_mean  a D > 1 mean tag summed pairwise (refine's mean; the matcher's centres)
#   row_mean       refine's mean taken from the tag columns of the rows, not from the tag map
#   no_fallback    D == 1: round(|d|) with no regard for an overflowing d * d
FAULTS = ("sequential", "float64", "fma", "no_tail", "pairwise_mean", "row_mean", "no_fallback")


def _sum_squares_fma(d):
    """sum of d * d over the last axis in the reference's order (sequential below 8, numpy's pairwise walk from 8),
    with every ``acc + d * d`` a fused multiply-add - what a compiler contracting the kernels' expressions would do"""
    D = d.shape[-1]
    col = [np.ascontiguousarray(d[..., k]) for k in range(D)]
    if D < 8:
        s = col[0] * col[0]
        for k in range(1, D):
            s = _fma32(col[k], col[k], s)
        return s
    r = [col[k] * col[k] for k in range(8)]
    i = 8
    while i + 8 <= D:
        for k in range(8):
            r[k] = _fma32(col[i + k], col[i + k], r[k])
        i += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < D:
        s = _fma32(col[i], col[i], s)
        i += 1
    return s


# --------------------------------------------------------------------------- #
# HeatmapParser
# --------------------------------------------------------------------------- #
class HeatmapParserRef:
    def __init__(self, num_joints=17, max_num_people=30, detection_threshold=0.1,
                 tag_threshold=1.0, use_detection_val=True, ignore_too_much=False,
                 tag_per_joint=True, nms_ksize=5, nms_padding=2, stable_topk=False):
        self.params = Params(num_joints, max_num_people, detection_threshold,
                             tag_threshold, use_detection_val, ignore_too_much)
        self.tag_per_joint = tag_per_joint
        self.nms_ksize, self.nms_padding = nms_ksize, nms_padding
        # False: torch.topk, what the reference runs (the goldens come from it).  True: the order the HIP decode
        # declares among equal values - a stable sort, lowest flat index first (``top_k_stable``)
        self.stable_topk = stable_topk

    def nms(self, det):
        """group.py:134-138: keep a pixel iff it equals its 5x5 window max"""
        m = F.max_pool2d(det, self.nms_ksize, 1, self.nms_padding)
        return det * torch.eq(m, det).float()

    def top_k(self, det, tag):
        """group.py:144-179.  det (N,J,h,w); tag (N,J,h,w,D) (or (N,1,h,w,D) if
        not tag_per_joint).  Order among equal values is whatever ATen gives (it is not the index order, and
        which members of a tie group at the K-th place are returned is not defined either); with
        ``stable_topk=True`` the selection is ``top_k_stable``'s: descending value, ascending flat index."""
        det = self.nms(det)
        N, J, h, w = det.shape
        if self.stable_topk:
            val_k, ind = self.top_k_stable(det)
        else:
            val_k, ind = det.reshape(N, J, -1).topk(self.params.max_num_people, dim=2)
        tag = tag.reshape(tag.shape[0], tag.shape[1], w * h, -1)
        if not self.tag_per_joint:
            tag = tag.expand(-1, self.params.num_joints, -1, -1)
        tag_k = torch.stack([torch.gather(tag[..., d], 2, ind) for d in range(tag.shape[3])], 3)
        x = ind % w
        y = (ind / w).long()          # true division then truncation, :168-169
        return {"tag_k": tag_k.numpy(), "loc_k": torch.stack((x, y), 3).numpy(),
                "val_k": val_k.numpy()}

    def top_k_stable(self, nms):
        """the K first entries of a stable descending sort of every NMS plane: ``np.argsort(-plane,
        kind="stable")[:K]``, so equal values (+0 and -0 are equal) come in ascending flat index.  nms (N,J,h,w)
        torch f32 -> (val_k (N,J,K) f32, ind (N,J,K) i64) torch tensors, as ``Tensor.topk`` returns them."""
        N, J, h, w = nms.shape
        K = self.params.max_num_people
        flat = nms.reshape(N * J, h * w).numpy()
        ind = np.stack([np.argsort(-row, kind="stable")[:K] for row in flat]).astype(np.int64)
        val = np.take_along_axis(flat, ind, 1)
        return torch.from_numpy(val.reshape(N, J, K)), torch.from_numpy(ind.reshape(N, J, K))

    def match(self, tag_k, loc_k, val_k, fault=None):
        return [match_by_tag(t, l, v, self.params, fault) for t, l, v in zip(tag_k, loc_k, val_k)]

    def adjust(self, ans, det):
        """group.py:181-200 quarter-pixel shift towards the larger neighbour;
        columns are compared first, then rows; ties and borders go to -0.25"""
        det = np.asarray(det)
        for b, people in enumerate(ans):
            for p in range(len(people)):
                for j in range(people.shape[1]):
                    if people[p, j, 2] > 0:
                        cx, cy = people[p, j, 0], people[p, j, 1]       # float32
                        col, row = int(cx), int(cy)
                        m = det[b, j]
                        H, W = m.shape
                        cx = cx + f32(0.25) if m[row, min(col + 1, W - 1)] > m[row, max(col - 1, 0)] \
                            else cx - f32(0.25)
                        cy = cy + f32(0.25) if m[min(row + 1, H - 1), col] > m[max(row - 1, 0), col] \
                            else cy - f32(0.25)
                        people[p, j, 0] = cx + f32(0.5)
                        people[p, j, 1] = cy + f32(0.5)
        return ans

    @staticmethod
    def refine_mean(tag, kp, fault=None):
        """group.py:214-222: the float32 mean tag of a person's detected joints, read from the tag MAP at
        ``(int(y), int(x))`` of the rows.  tag (J,h,w,D), kp (J,3+D).  ``fault`` (see ``FAULTS``): "row_mean" takes
        the tags from columns 3.. of the rows instead, "pairwise_mean" sums them pairwise also for D > 1."""
        J, D = tag.shape[0], tag.shape[3]
        if fault == "row_mean":
            seen = [kp[j, 3:] for j in range(J) if kp[j, 2] > 0]
        else:
            seen = [tag[j, int(kp[j, 1]), int(kp[j, 0])] for j in range(J) if kp[j, 2] > 0]
        seen = np.asarray(seen, f32)                       # (n, D)
        if D == 1 or fault == "pairwise_mean":
            return np.array([pairwise8_sum_f32(seen[:, d]) / f32(len(seen)) for d in range(D)], f32)
        s = np.zeros(D, f32)
        for t in seen:
            s = (s + t).astype(f32)
        return (s / f32(len(seen))).astype(f32)

    @staticmethod
    def refine_score(det_j, tag_j, mean, fault=None):
        """group.py:229-232: the map whose first maximum refine takes, heat value minus the rounded tag distance.
        det_j (h,w), tag_j (h,w,D), mean (D,).  ``fault``: one of the wrong summation orders of ``FAULTS``."""
        D = tag_j.shape[2]
        with np.errstate(over="ignore", invalid="ignore"):
            d = tag_j - mean[None, None, :]
            if fault == "no_fallback" and D == 1:          # round(|d|): equal to the reference unless d * d overflows
                return det_j - np.rint(np.abs(d[..., 0]))
            if fault == "float64":
                ss = np.zeros(d.shape[:2], np.float64)
                for k in range(D):
                    ss = ss + d[..., k].astype(np.float64) ** 2
                return det_j - np.rint(np.sqrt(ss))
            if fault == "fma":
                return det_j - np.rint(np.sqrt(_sum_squares_fma(d)))
            sq = d * d
            if fault == "no_tail" and D >= 8:
                sq = np.ascontiguousarray(sq[..., :D // 8 * 8])
                D = sq.shape[2]
            if D < 8 or fault == "sequential":
                ss = sq[..., 0].copy()
                for k in range(1, D):
                    ss = ss + sq[..., k]
            else:
                ss = sq.sum(axis=2)                        # numpy pairwise, as the reference
            return det_j - np.rint(np.sqrt(ss))            # np.round == half-to-even

    def refine(self, det, tag, kp, fault=None, means=None):
        """group.py:202-264 for one person.  det (J,h,w) f32, tag (J,h,w,D) f32,
        kp (J,3+D) f32 (modified in place and returned).  ``fault``: see ``FAULTS``; ``means``: per joint the mean
        tag to use instead of the person's own (the seeded slot mix-up of oracle/tagdims.py)."""
        if tag.ndim == 3:
            tag = tag[..., None]
        J, h, w = det.shape
        mean = self.refine_mean(tag, kp, fault)
        for j in range(J):
            if kp[j, 2] != 0:                              # only undetected joints are filled: nothing to decide here
                continue
            score = self.refine_score(det[j], tag[j], mean if means is None else means[j], fault)
            flat = int(np.argmax(score))                   # first maximum
            y, x = divmod(flat, w)
            val = det[j, y, x]
            fx = x + 0.5 + (0.25 if det[j, y, min(x + 1, w - 1)] > det[j, y, max(x - 1, 0)] else -0.25)
            fy = y + 0.5 + (0.25 if det[j, min(y + 1, h - 1), x] > det[j, max(y - 1, 0), x] else -0.25)
            if val > 0:
                kp[j, 0], kp[j, 1], kp[j, 2] = fx, fy, val
        return kp

    def parse(self, det, tag, adjust=True, refine=True):
        """group.py:266-287.  det (N,J,h,w) torch f32; tag (N,J,h,w,D)."""
        ans = self.match(**self.top_k(det, tag))
        det_np = det.numpy()
        if adjust:
            ans = self.adjust(ans, det_np)
        scores = [pairwise8_sum_f32(np.ascontiguousarray(p[:, 2])) / f32(len(p[:, 2]))
                  for p in ans[0]]
        if refine:
            people = ans[0]
            tag_np = tag[0].numpy()
            if not self.tag_per_joint:
                tag_np = np.tile(tag_np, (self.params.num_joints, 1, 1, 1))
            for p in range(len(people)):
                people[p] = self.refine(det_np[0], tag_np, people[p])
            ans = [people]
        return ans, scores


def match_by_tag(tag_k, loc_k, val_k, P, fault=None):
    """group.py:26-97 for one image.  tag_k (J,K,D) f32, loc_k (J,K,2) i64,
    val_k (J,K) f32 -> (P, J, 3+D) float32 (shape (0,) if nobody found).  ``fault``: "sequential" (the distances)
    or "pairwise_mean" (the centres) of ``FAULTS``."""
    J, D = P.num_joints, tag_k.shape[2]
    people = OrderedDict()      # key = float value of tag[0] -> [rows (J,3+D) f64, [tags f32]]

    def put(key, j, row, t):
        # dict.setdefault semantics of :51-52 / :91-94: an existing key keeps
        # its rows but its tag list is reset
        if key not in people:
            people[key] = [np.zeros((J, 3 + D)), None]
        people[key][0][j] = row
        people[key][1] = [t]

    for j in range(J):
        rows = np.concatenate((loc_k[j].astype(np.float64),
                               val_k[j][:, None].astype(np.float64),
                               tag_k[j].astype(np.float64)), 1)
        keep = rows[:, 2] > P.detection_threshold
        rows, tags = rows[keep], tag_k[j][keep]
        if not len(rows):
            continue
        if j == 0 or not people:
            for t, r in zip(tags, rows):
                put(t[0], j, r, t)
            continue
        keys = list(people)[:P.max_num_people]
        if P.ignore_too_much and len(keys) == P.max_num_people:
            continue
        centres = np.stack([_mean_tags_f32(people[k][1], fault == "pairwise_mean") for k in keys])     # (G, D) f32
        diff = rows[:, None, 3:] - centres[None].astype(np.float64)
        dist = np.sqrt(_sum_last_f64(diff * diff, fault == "sequential"))                         # (A, G)
        cost = np.rint(dist) * 100 - rows[:, 2:3] if P.use_detection_val else dist.copy()
        A, G = dist.shape
        if A > G:
            cost = np.concatenate((cost, np.full((A, A - G), 1e10)), 1)
        for r, c in munkres_compute(cost):
            if r < A and c < G and dist[r, c] < P.tag_threshold:
                people[keys[c]][0][j] = rows[r]
                people[keys[c]][1].append(tags[r])
            else:
                put(tags[r][0], j, rows[r], tags[r])
    return np.array([v[0] for v in people.values()]).astype(f32)


def _mean_tags_f32(tags, pairwise=False):
    """np.mean(list of (D,) f32, axis=0), group.py:55 (``pairwise``: the seeded fault)"""
    a = np.asarray(tags, f32)
    n = f32(len(a))
    if a.shape[1] == 1 or pairwise:
        return np.array([pairwise8_sum_f32(a[:, d]) / n for d in range(a.shape[1])], f32)
    s = np.zeros(a.shape[1], f32)
    for t in a:
        s = (s + t).astype(f32)
    return (s / n).astype(f32)


def _sum_last_f64(a, sequential=False):
    """add.reduce over the contiguous last axis, float64 (np.linalg.norm :62; ``sequential``: the seeded fault)"""
    D = a.shape[-1]
    if D < 8 or sequential:
        s = a[..., 0].copy()
        for k in range(1, D):
            s = s + a[..., k]
        return s
    return a.sum(axis=-1)
