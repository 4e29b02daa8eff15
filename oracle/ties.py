"""Decode inputs with exact ties by construction, and the counters that prove the ties are there (oracle; test
infrastructure only, see oracle/__init__.py).

The HIP decode declares an order among equal values - lowest flat index first, on every top-k and arg-max path - that
``torch.topk`` does not define; ``HeatmapParserRef(stable_topk=True)`` is the yardstick.  The maps made here carry
values from small dyadic sets, so that equal maxima, plateaus, tie groups at the K-th place and equal refine scores
exist exactly, also after the exact upsamplings the fused paths apply (identity, ``out = 2 * in - 1`` with
align_corners=True, the 2x / 4x / 8x projections with align_corners=False).  Nothing here is trusted: the callers push
every scene through the CPU upsampling and hand the result to ``topk_structure`` / ``refine_structure``, which COUNT
what is present.

Two kinds of scene:

* ``direct_scene``: 17 planes of (160, 224) with one designed structure per plane (see its docstring) - the
  already-upsampled maps of ``parse`` / ``top_k``, and the ``refined`` input of ``parse_lowres`` at ``out_hw`` equal to
  the map size or to ``2 * in - 1``;
* ``lattice_scene``: translated copies of single pixels and aligned plateaus on a coarse lattice, rendered at any
  number of pixels per cell - the network-shaped inputs of the flip / multi-scale paths and of the per-image sizes.
"""
import numpy as np
import torch

from . import decode_ref, inference_ref

f32 = np.float32
J = 17
TH, TW = 32, 64                      # the tile of the top-k kernels (csrc/decode.hip kTH, kTW)
SCAN_STRIPES, ARGMAX_STRIPES = 10, 20   # row stripes of refine's scan and of the plane-maximum pass
ARGMAX_THREADS, ARGMAX_COLS = 256, 8    # the plane-maximum pass: threads per block, columns a thread owns at the most
PERSON_TAGS = (3.0, 6.0, 9.0, 12.0)  # persons A-D; every other tag is >= 50
EPS = 0.0625                         # the smallest positive value of the dyadic set: below the detection threshold 0.1


def _bg_tags(rng, shape):
    """dyadic background tags in [50, 60): far from every person, many equal pairs"""
    return (50 + rng.integers(0, 80, shape) / 8.0).astype(f32)


def _block(tag, y, x, value, r=6):
    tag[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = value


# --------------------------------------------------------------------------- #
# the designed scene
# --------------------------------------------------------------------------- #
DIRECT_HW = (160, 224)


def direct_scene(K=30, seed=0):
    """det (17,160,224) f32, tag (17,160,224) f32.  Planes (persons A-D carry the tags 3, 6, 9, 12):

    0      the four persons' peaks, all 1.0: A and B in one tile, C in the next tile of the row, D two tile rows down
    1      K - 3 peaks above 0.5 and eight peaks of exactly 0.5 scattered over the tiles: a tie group at the K-th place
    2      a 24x32 plateau of 0.75 inside one tile (768 local maxima) and a 4x6 plateau of 1.0 across a tile corner
    3, 9   the plane maximum 0.0625 (below the detection threshold: everybody misses the joint) at three pixels in
           different row stripes, on borders and in corners, tagged for A, B and D (C: no penalty-free pixel); and
           behind the first of them further such pixels that ONE thread of the plane-maximum pass meets in ONE of its
           row stripes (see ``walk_thread``): on plane 3 at 256 and 512 flat pixels from it, tagged for B and for A
           (the walk over flat indices), on plane 9 in its column three and seven rows down, tagged for B and for A
           (the walk over columns)
    4, 5   refine score ties between different heat values: 1.0625 with penalty 1 against 0.0625 with penalty 0,
           both orders, in one stripe (plane 4) and in different stripes (plane 5)
    6, 7   single-pixel peaks of 1.0 in every corner and on every border
    8      negative values, exact zeros, -0.0, five equal positive peaks and three others: fewer than K positives
    10-16  the persons' peaks with pairwise equal values, half of them with unequal neighbours
    """
    h, w = DIRECT_HW
    rng = np.random.default_rng(1000 + seed)
    det = np.zeros((J, h, w), f32)
    tag = _bg_tags(rng, (J, h, w))
    home = ((10, 10), (10, 40), (10, 100), (100, 30))

    def peak(j, y, x, v, person=None, asym=False):
        det[j, y, x] = v
        if asym:          # left > right, down > up: adjust goes -0.25 in x, +0.25 in y
            det[j, y, x - 1], det[j, y, x + 1] = v / 2, v / 4
            det[j, y - 1, x], det[j, y + 1, x] = v / 4, v / 2
        if person is not None:
            _block(tag[j], y, x, PERSON_TAGS[person])

    for p, (y, x) in enumerate(home):                                   # plane 0
        peak(0, y, x, 1.0, p)
    # plane 1: the tie group at the K-th place
    slots = [(y, x) for y in range(6, h - 3, 12) for x in range(6, w - 3, 12)]
    order = rng.permutation(len(slots))
    n_high = max(K - 3, 0)
    for i in range(n_high):
        y, x = slots[order[i]]
        det[1, y, x] = 0.5 + (i % 96 + 1) / 64.0
    for i in range(8):
        y, x = slots[order[n_high + i]]
        det[1, y, x] = 0.5
    # plane 2: plateaus
    det[2, 34:58, 66:98] = 0.75
    det[2, 94:98, 189:195] = 1.0
    # planes 3 and 9: a tied plane maximum nobody detects
    for j, pix in ((3, ((0, 0), (70, w - 1), (h - 1, 100))), (9, ((0, 120), (90, 0), (h - 1, 0)))):
        for (y, x), person in zip(pix, (0, 1, 3)):
            peak(j, y, x, EPS, person)
        det[j, 40:50, 30:200] = -(rng.integers(1, 9, (10, 170)) / 16.0).astype(f32)
    assert w + 32 == ARGMAX_THREADS                     # 256 flat pixels = one row down and 32 columns on
    peak(3, 1, 32, EPS, 1)
    peak(3, 2, 64, EPS, 0)
    det[9, 3, 120] = det[9, 7, 120] = EPS               # rows 0, 3, 7 of one column: A, B, A (the tags of the rows
    tag[9, 2:5, 114:127] = PERSON_TAGS[1]               # around, as the half-resolution tag maps keep every other row)
    tag[9, 5:10, 114:127] = PERSON_TAGS[0]
    # planes 4 and 5: score ties between a high pixel with penalty 1 and a low one with penalty 0
    hi, lo = 1.0 + EPS, EPS

    def pair(j, person, first, second, high_first):
        (y0, x0), (y1, x1) = first, second
        t = PERSON_TAGS[person]
        det[j, y0, x0], det[j, y1, x1] = (hi, lo) if high_first else (lo, hi)
        _block(tag[j], y0, x0, t + 1.25 if high_first else t)
        _block(tag[j], y1, x1, t if high_first else t + 1.25)
    pair(4, 0, (40, 50), (42, 120), True)
    pair(4, 1, (100, 40), (102, 150), False)
    peak(4, 130, 60, 1.0, 2)
    peak(4, 140, 180, 0.75, 3)
    pair(5, 2, (20, 60), (120, 70), True)
    pair(5, 3, (60, 150), (140, 160), False)
    peak(5, 80, 20, 1.0, 0)
    peak(5, 85, 200, 1.0, 1)
    # planes 6 and 7: borders and corners
    for j, pix in ((6, ((0, 0), (0, 100), (80, 0), (h - 1, w - 1))), (7, ((60, w - 1), (h - 1, 90), (0, w - 1), (h - 1, 0)))):
        for p, (y, x) in enumerate(pix):
            peak(j, y, x, 1.0, p)
    # plane 8: negatives, zeros, -0.0 and a few positives
    det[8] = -(rng.integers(1, 17, (h, w)) / 16.0).astype(f32)
    det[8, 3:6, 20:90] = 0.0
    det[8, 1, 40:44] = -0.0
    det[8, 0, 3] = det[8, 0, 12] = -1 / 32.0            # negative local maxima among the first pixels, at any window
    det[8, 60:70, :] = 0.0
    for p, (y, x) in enumerate(((30, 30), (30, 150), (110, 60), (120, 190))):
        peak(8, y, x, 0.5, p)
    for (y, x), v in (((64, 100), 0.5), ((64, 20), 0.75), ((64, 200), 1.25), ((130, 120), 0.25)):
        det[8, y, x] = v
    # planes 10-16: the persons again, values equal in pairs
    for j in range(10, J):
        vals = np.roll((1.0, 1.0, 0.75, 0.75), j)
        for p, (y, x) in enumerate(home):
            peak(j, y + 4 * (j - 8), x + 5 * (j - 8), float(vals[p]), p, asym=(j + p) % 2 == 0)
    return det, tag


def direct_inputs(K=30, seed=0, D=1):
    """the scene as ``parse`` takes it: det (1,17,h,w), tag (1,17,h,w,D) torch f32; the channels d >= 1 carry a
    pixel-dependent pattern of at most 7/64, too small to change a rounded tag distance"""
    det, tag = direct_scene(K, seed)
    jj, yy, xx = np.meshgrid(np.arange(J), np.arange(det.shape[1]), np.arange(det.shape[2]), indexing="ij")
    pattern = ((yy * 31 + xx * 17 + jj) % 8 / 64.0).astype(f32)
    tags = np.stack([tag if d == 0 else pattern * f32(d) for d in range(D)], axis=-1)
    return torch.from_numpy(det[None]), torch.from_numpy(np.ascontiguousarray(tags[None]))


def lowres_inputs(K=30, seeds=(0,)):
    """the scene as ``parse_lowres`` takes it: refined (N,17,160,224) and tags (N,17,80,112) torch f32, one image
    per seed; to be decoded at (160, 224) or at (319, 447)"""
    scenes = [direct_scene(K, s) for s in seeds]
    refined = np.stack([s[0] for s in scenes])
    tags = np.stack([s[1][:, ::2, ::2] for s in scenes])
    return torch.from_numpy(refined), torch.from_numpy(np.ascontiguousarray(tags))


def upsampled(refined, tags, out_hw):
    """what the reference builds from the network outputs (validate_hhrnet.py:94-98): (N,J,oh,ow), (N,J,oh,ow,1)"""
    hms = decode_ref.upsample_bilinear(refined, out_hw[0], out_hw[1])
    aes = decode_ref.upsample_bilinear(tags, out_hw[0], out_hw[1])
    return hms, aes.unsqueeze(-1)


def big_map(seed=0):
    """det (1,3,1500,3000), tag (1,3,1500,3000,1): 47 x 47 = 2,209 tiles per plane.  Plane 0: 200 peaks of eight
    dyadic levels (every level a tie group, one of them at the K-th place for K = 8 and K = 30); plane 1: five equal
    peaks in an otherwise negative plane (zero padding behind ties); plane 2: a plateau across a tile corner and
    equal peaks"""
    h, w = 1500, 3000
    rng = np.random.default_rng(77 + seed)
    det = np.zeros((3, h, w), f32)
    ys, xs = rng.permutation(np.arange(8, h - 8, 12))[:100], rng.permutation(np.arange(8, w - 8, 12))[:200]
    for i in range(200):
        det[0, ys[i % 100] + (i // 100) * 4, xs[i]] = (8 - i % 8) / 8.0
    det[1] = -(rng.integers(1, 17, (h, w)) / 16.0).astype(f32)
    for y, x in ((5, 2990), (700, 1500), (700, 10), (1490, 40), (1200, 2222)):
        det[1, y, x] = 0.5
    det[2, 31:33, 63:65] = 1.0
    for i in range(40):
        det[2, ys[i], xs[i]] = 0.75
    tag = rng.integers(0, 1 << 20, (3, h, w, 1)).astype(f32)
    return torch.from_numpy(det[None]), torch.from_numpy(tag[None])


# --------------------------------------------------------------------------- #
# lattice scenes: translated copies, rendered at any resolution
# --------------------------------------------------------------------------- #
def lattice_scene(gh, gw, seed=0, n_peaks=38, plateau=True):
    """an abstract scene on a (gh, gw) lattice: per plane a list of ``(cy, cx, amplitude)`` peaks at lattice points
    at least 3 cells apart and 2 cells from the border, amplitudes from four dyadic levels (so every level is a tie
    group of translated copies), on the planes j % 4 == 2 a plateau of whole cells; the four persons own the first
    peaks of every plane but 1-3 (tags 3, 6, 9, 12 on the cells around), every other cell carries a background tag"""
    rng = np.random.default_rng(500 + seed)
    slots = [(y, x) for y in range(2, gh - 2, 3) for x in range(2, gw - 2, 3)]
    peaks, plats = [], []
    tagc = _bg_tags(rng, (J, gh, gw))
    for j in range(J):
        rect = None
        if plateau and j % 4 == 2:
            rect = (gh // 2 - 1, gh // 2 + 4, gw // 2 - 2, gw // 2 + 6, 0.75)
        plats.append(rect)
        free = [s for s in slots if rect is None or not (rect[0] - 2 <= s[0] < rect[1] + 2 and rect[2] - 2 <= s[1] < rect[3] + 2)]
        order = rng.permutation(len(free))
        n = min(n_peaks, len(free)) if j % 4 != 3 else 6
        pl = []
        for i in range(n):
            cy, cx = free[order[i]]
            pl.append((cy, cx, (4 - i % 4) / 4.0))
            if i < 4 and j not in (1, 2, 3):
                tagc[j, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = PERSON_TAGS[i]
        peaks.append(pl)
    return dict(gh=gh, gw=gw, peaks=peaks, plateaus=plats, tags=tagc)


def render(scene, r, amp=1.0):
    """heat maps (17, gh*r, gw*r) f32 at r pixels per cell: a peak is ONE pixel at (cy*r, cx*r), a plateau the
    pixels of its cells"""
    det = np.zeros((J, scene["gh"] * r, scene["gw"] * r), f32)
    for j in range(J):
        if scene["plateaus"][j] is not None:
            y0, y1, x0, x1, v = scene["plateaus"][j]
            det[j, y0 * r:y1 * r, x0 * r:x1 * r] = v * amp
        for cy, cx, a in scene["peaks"][j]:
            det[j, cy * r, cx * r] = a * amp
    return det


def render_tags(scene, r):
    """tag maps (17, gh*r, gw*r) f32: constant on every cell"""
    return np.ascontiguousarray(np.repeat(np.repeat(scene["tags"], r, axis=1), r, axis=2))


def sizes_inputs(seeds=(0, 1, 2, 3)):
    """per-image sizes: refined (N,17,48,80), tags (N,17,24,40) - a (24, 40) lattice at 2 and 1 pixels per cell"""
    sc = [lattice_scene(24, 40, s, n_peaks=36) for s in seeds]
    refined = np.stack([render(s, 2) for s in sc])
    tags = np.stack([render_tags(s, 1) for s in sc])
    return torch.from_numpy(refined), torch.from_numpy(tags)


NET_HW = (256, 384)          # the scale-1 input size of the flip / multi-scale scenes: a (32, 48) lattice of 8 px cells


def net_outputs(N, scales, seed=0):
    """per scale (descending) the teacher-shaped outputs ``(preds (N,34,H*s/4,W*s/4), refined (N,17,H*s/2,W*s/2),
    preds_f, refined_f)`` of one lattice scene per image: a cell is 8 output pixels, so it is 4*s refined and 2*s
    preds pixels wide and every peak is a single pixel at every resolution.  The mirror image's outputs are the
    mirrored maps with left / right joints swapped, the heat maps halved and the tags moved by 0.25 (all exact)."""
    H, W = NET_HW
    perm = inference_ref.FLIP_COCO
    scenes = [lattice_scene(H // 8, W // 8, seed + 10 * n) for n in range(N)]
    outs = []
    for s in sorted(scales, reverse=True):
        r2, r4 = int(4 * s), int(2 * s)
        assert r2 == 4 * s and r4 == 2 * s and r4 >= 1
        R = torch.from_numpy(np.stack([render(sc, r2) for sc in scenes]))
        Ph = np.stack([render(sc, r4, amp=0.5) for sc in scenes])
        Pt = np.stack([render_tags(sc, r4) for sc in scenes])
        P = torch.from_numpy(np.concatenate([Ph, Pt], axis=1))
        Pf = torch.flip(P, [3])[:, perm + [J + q for q in perm]].clone()
        Pf[:, :J] *= 0.5
        Pf[:, J:] += 0.25
        Rf = torch.flip(R, [3])[:, perm] * 0.5
        outs.append(tuple(t.contiguous() for t in (P, R, Pf, Rf)))
    return outs


def net_maps(outs, scales, flip, n, ags=False):
    """image n through the torch-CPU restatement of the multi-scale / flip aggregation (oracle/inference_ref.py):
    the projected heat maps (1,17,H,W) and tags (1,17,H,W,1+flip) - with ``ags`` the ONE tag map (1,1,H,W,1) of the
    AGS branch: channel 0 of the un-mirrored tag maps of the smallest scale"""
    H, W = NET_HW
    order = sorted(scales, reverse=True)
    store = {s: o for s, o in zip(order, outs)}
    calls = {}

    def model(image):
        s = float(image[0, 0, 0, 0].item())            # the stand-in input carries its scale
        k = calls.get(s, 0)
        calls[s] = k + 1
        P, R, Pf, Rf = store[s]
        return [t[n:n + 1].clone() for t in ((P, R) if k % 2 == 0 or not flip else (Pf, Rf))]
    inputs = {s: torch.full((1, 3, 8, 8), float(s)) for s in order}
    hm, tags = inference_ref.multi_scale_maps(model, inputs, order, (W, H), flip, True)
    if ags:
        calls.clear()
        _, _, tl = inference_ref.get_multi_stage_outputs(model, inputs[min(order)], flip, True, (W, H))
        tags = tl[0][:, 0].unsqueeze(-1).unsqueeze(0)
    return hm, tags


# --------------------------------------------------------------------------- #
# counters
# --------------------------------------------------------------------------- #
def topk_structure(nms_plane, K):
    """what a stable top-K of one NMS plane (h, w) holds: ``groups`` [(value, members)] of equal positive values
    inside the top K; how many of them have two members in one tile (``same_tile``), members in different tiles
    (``other_tile``), in different tile rows (``other_tile_row``), in the four tiles around one tile corner
    (``corner4``); ``straddle`` = (value, taken, total, lowest_taken) if the K-th value is positive and more pixels
    carry it than rows were left; ``tile_maxima`` = the largest number of positive local maxima in one tile;
    ``positives``; ``padding`` = the flat indices of the zero-valued rows"""
    nms_plane = np.asarray(nms_plane)
    h, w = nms_plane.shape
    flat = nms_plane.reshape(-1)
    order = np.argsort(-flat, kind="stable")[:K]
    vals = flat[order]
    out = dict(groups=[], same_tile=0, other_tile=0, other_tile_row=0, corner4=0, straddle=None)
    for v in np.unique(vals[vals > 0]):
        idx = order[vals == v]
        if len(idx) < 2:
            continue
        tiles = list(zip((idx // w // TH).tolist(), (idx % w // TW).tolist()))
        ts = set(tiles)
        out["groups"].append((float(v), len(idx)))
        out["same_tile"] += len(ts) < len(tiles)
        out["other_tile"] += len(ts) >= 2
        out["other_tile_row"] += len(set(t[0] for t in ts)) >= 2
        out["corner4"] += any({(a, b), (a, b + 1), (a + 1, b), (a + 1, b + 1)} <= ts for a, b in ts)
    vk = vals[K - 1]
    if vk > 0:
        total, taken = int((flat == vk).sum()), int((vals == vk).sum())
        if total > taken:
            all_idx = np.flatnonzero(flat == vk)
            out["straddle"] = (float(vk), taken, total, bool(np.array_equal(order[vals == vk], all_idx[:taken])))
    pos = nms_plane > 0
    ph, pw = -(-h // TH) * TH, -(-w // TW) * TW
    padded = np.zeros((ph, pw), np.int64)
    padded[:h, :w] = pos
    out["tile_maxima"] = int(padded.reshape(ph // TH, TH, pw // TW, TW).sum(axis=(1, 3)).max())
    out["tiles"] = (ph // TH) * (pw // TW)
    out["positives"] = int(pos.sum())
    out["padding"] = order[vals == 0]
    return out


def _where(y, x, h, w):
    ey, ex = y in (0, h - 1), x in (0, w - 1)
    if ey and ex:
        return "corner"
    if ey:
        return "top" if y == 0 else "bottom"
    if ex:
        return "left" if x == 0 else "right"
    return "interior"


def _equal_neighbours(m, y, x):
    """no larger neighbour to pick on either axis: the two neighbours are equal, or the keypoint sits on the border
    of that axis (the clamped neighbour is the keypoint itself, which the other one cannot exceed at a maximum)"""
    h, w = m.shape
    return (x in (0, w - 1) or m[y, x + 1] == m[y, x - 1]) and (y in (0, h - 1) or m[y + 1, x] == m[y - 1, x])


def walk_thread(idx, h, w, walk):
    """(row stripe, thread) of the plane-maximum pass that meets the pixels ``idx`` (flat, ascending) of an (h, w)
    plane.  A block of 256 threads takes one of 20 row stripes; ``walk`` "flat": thread t meets the stripe's flat
    pixels t, t + 256, ... (already-upsampled maps, and maps wider than 2,048); "column": thread t owns the columns
    t, t + 256, ... and goes down the rows (the fused bilinear maps)."""
    idx = np.asarray(idx)
    ra = -(-h // ARGMAX_STRIPES)
    stripe = idx // w // ra
    if walk == "column" and w <= ARGMAX_THREADS * ARGMAX_COLS:
        return stripe, idx % w % ARGMAX_THREADS
    return stripe, (idx - stripe * ra * w) % ARGMAX_THREADS


def last_met(top, h, w, walk):
    """the pixel a plane-maximum pass would report that kept, of the equal maxima ``top`` ONE thread meets in ONE
    stripe, the last instead of the first: threads and stripes are merged by lowest index whatever a thread did, so
    this - and not the last of all - is what such a fault returns.  Equal to ``top[0]`` unless the first maximum
    shares its stripe and thread with a later one."""
    last = {}
    for i, s, t in zip(np.asarray(top).tolist(), *[a.tolist() for a in walk_thread(top, h, w, walk)]):
        last[(s, t)] = i
    return min(last.values())


def refine_structure(det, tag, matched):
    """counts over one image's people BEFORE adjust / refine (``matched`` (P,J,3+D), the oracle's ``match`` rows;
    det (J,h,w), tag (J,h,w,D) numpy): for every missing joint the oracle's own score map is looked at.

    ``max_first`` / ``max_later`` / ``max_none``: (person, joint) pairs whose plane maximum is positive and attained
    at several pixels lying in different row stripes, with tag penalty 0 at the first of them / not at the first but
    at a later one / at none.  ``same_thread`` / ``same_thread_later``, by walk ("flat", "column", see
    ``walk_thread``): pairs whose first plane maximum shares its stripe AND thread of the plane-maximum pass with
    later ones, with penalty 0 at the first and at the one ``last_met`` names (a thread that kept its last maximum
    moves this person's joint there) / with penalty 0 not at the first but at a later one of that thread.  ``score_ties``: pairs whose best score is attained at pixels of DIFFERENT heat values,
    keyed by (higher value first?, same scan stripe?).  ``missing``: the largest number of people missing one joint
    among the joints that have such a tie.  ``adjust_equal`` / ``refine_equal``: detected / filled joints with equal
    left-right and equal up-down neighbours (or none, on a border), by place (interior, top, bottom, left, right, corner);
    ``adjust_unequal``: detected joints with an unequal pair of neighbours."""
    ref = decode_ref.HeatmapParserRef
    Jn, h, w = det.shape
    rs, ra = -(-h // SCAN_STRIPES), -(-h // ARGMAX_STRIPES)
    out = dict(max_first=0, max_later=0, max_none=0, score_ties={}, missing=0, adjust_equal={}, refine_equal={},
               adjust_unequal=0, same_thread=dict(flat=0, column=0), same_thread_later=dict(flat=0, column=0))
    tie_joints = set()
    for kp in matched:
        mean = ref.refine_mean(tag, kp)
        for j in range(Jn):
            if kp[j, 2] > 0:
                y, x = int(kp[j, 1]), int(kp[j, 0])
                if _equal_neighbours(det[j], y, x):
                    k = _where(y, x, h, w)
                    out["adjust_equal"][k] = out["adjust_equal"].get(k, 0) + 1
                else:
                    out["adjust_unequal"] += 1
                continue
            score = ref.refine_score(det[j], tag[j], mean)
            pen = det[j] - score
            best = np.flatnonzero(score.reshape(-1) == score.max())
            y, x = divmod(int(best[0]), w)
            if det[j, y, x] > 0 and _equal_neighbours(det[j], y, x):
                k = _where(y, x, h, w)
                out["refine_equal"][k] = out["refine_equal"].get(k, 0) + 1
            top = np.flatnonzero(det[j].reshape(-1) == det[j].max())
            if det[j].max() > 0 and len(set((top // w // rs).tolist())) > 1 and len(set((top // w // ra).tolist())) > 1:
                p = pen.reshape(-1)[top]
                out["max_first" if p[0] == 0 else "max_later" if (p == 0).any() else "max_none"] += 1
                tie_joints.add(j)
            if det[j].max() > 0 and len(top) > 1:
                p = pen.reshape(-1)
                for walk in ("flat", "column"):
                    stripe, thread = walk_thread(top, h, w, walk)
                    mates = top[(stripe == stripe[0]) & (thread == thread[0])][1:]
                    q = last_met(top, h, w, walk)
                    out["same_thread"][walk] += bool(q != top[0] and p[top[0]] == 0 and p[q] == 0)
                    out["same_thread_later"][walk] += bool(p[top[0]] != 0 and (p[mates] == 0).any())
            dv = det[j].reshape(-1)[best]
            if len(best) > 1 and dv.max() > dv.min() and dv[0] > 0:
                key = (bool(dv[0] == dv.max()), len(set((best // w // rs).tolist())) == 1)
                out["score_ties"][key] = out["score_ties"].get(key, 0) + 1
                tie_joints.add(j)
    for j in tie_joints:
        out["missing"] = max(out["missing"], int(sum(1 for kp in matched if kp[j, 2] == 0)))
    return out


def summarize(ref, hms, aes, n=0):
    """every count of image ``n`` of already-upsampled maps: ``planes`` (``topk_structure`` per plane), their sums
    (``same_tile`` ... ``straddles``, ``groups``, ``tile_maxima``), ``refine`` (``refine_structure`` on the stable
    oracle's own ``match`` rows) and ``people``.  ``ref``: a ``HeatmapParserRef(stable_topk=True)``."""
    K = ref.params.max_num_people
    nms = ref.nms(hms[n:n + 1])[0].numpy()
    planes = [topk_structure(p, K) for p in nms]
    out = dict(planes=planes, nms=nms, K=K)
    for k in ("same_tile", "other_tile", "other_tile_row", "corner4"):
        out[k] = sum(p[k] for p in planes)
    out["groups"] = sum(len(p["groups"]) for p in planes)
    out["straddles"] = [(j,) + p["straddle"] for j, p in enumerate(planes) if p["straddle"] is not None]
    out["tile_maxima"] = max(p["tile_maxima"] for p in planes)
    tag = aes[n if aes.shape[0] > 1 else 0].numpy()
    if tag.shape[0] == 1:
        tag = np.tile(tag, (nms.shape[0], 1, 1, 1))
    matched = ref.match(**ref.top_k(hms[n:n + 1], aes[n:n + 1] if aes.shape[0] > 1 else aes))[0]
    out["people"] = len(matched)
    out["refine"] = refine_structure(hms[n].numpy(), tag, matched) if len(matched) else None
    return out


PLACES = ("interior", "top", "bottom", "left", "right", "corner")


def require_designed(s, scaled=False):
    """the structures a-h of the issue on the designed scene, counted on the oracle's result (``s = summarize(...)``
    of the scene as it is, or ``scaled``: upsampled to 2 * in - 1).  Returns the counts worth recording."""
    K, pl = s["K"], s["planes"]
    rec = {}
    # b: the tie group at the K-th place of plane 1: min(3, K) of the eight taken, the lowest indices
    v, taken, total, lowest = pl[1]["straddle"]
    assert (v, taken, total, lowest) == (0.5, min(3, K), 8, True), pl[1]["straddle"]
    assert all(st[4] for st in s["straddles"]), s["straddles"]
    rec["b"] = [st[:4] for st in s["straddles"]]
    # c: more local maxima in one tile than the rank sort holds
    assert pl[2]["tile_maxima"] > 512 and pl[2]["straddle"] is not None, pl[2]
    rec["c_tile_maxima"] = pl[2]["tile_maxima"]
    if K < 30:
        return rec
    # a: equal maxima inside the top K: in one tile, in other tiles, in other tile rows
    assert (1.0, 4) in pl[0]["groups"] and pl[0]["other_tile"] and pl[0]["other_tile_row"], pl[0]
    assert s["same_tile"] >= 1 and (scaled or pl[0]["same_tile"]), s["same_tile"]
    rec["a"] = dict(groups=s["groups"], same_tile=s["same_tile"], other_tile=s["other_tile"],
                    other_tile_row=s["other_tile_row"])
    if not scaled or K >= 64:
        assert pl[2]["corner4"] >= 1, pl[2]            # c: one plateau in the four tiles around a corner
        rec["c_corner4"] = pl[2]["corner4"]
    r = s["refine"]
    # e: a tied plane maximum in different stripes; penalty 0 at the first, at a later one only, at none
    assert r["max_first"] >= 1 and r["max_later"] >= 1 and r["max_none"] >= 1, r
    # ... and several of them met by one thread in one stripe of the plane-maximum pass, on the walk over columns
    # (fused maps) and, at the scene's own size, on the walk over flat indices (already-upsampled maps)
    for walk in ("column",) if scaled else ("column", "flat"):
        assert r["same_thread"][walk] >= 1 and r["same_thread_later"][walk] >= 1, (walk, r)
    # f: equal scores from different heat values, both orders, in one stripe and across stripes; > 16 people scanned
    assert all(r["score_ties"].get((a, b), 0) >= 1 for a in (True, False) for b in (True, False)), r["score_ties"]
    assert r["missing"] > 16, r["missing"]
    # g: the quarter-pixel step without a larger neighbour, everywhere; and with one, so that '>' is told from '>='
    assert all(r["adjust_equal"].get(k, 0) >= 1 for k in PLACES), r["adjust_equal"]
    assert all(r["refine_equal"].get(k, 0) >= 1 for k in PLACES), r["refine_equal"]
    assert r["adjust_unequal"] >= 1
    rec["efg"] = {k: r[k] for k in ("max_first", "max_later", "max_none", "same_thread", "same_thread_later",
                                    "score_ties", "missing", "adjust_equal", "refine_equal", "adjust_unequal")}
    # h: negatives, both zeros, a tie group, fewer than K positives: the padding follows in index order and skips
    # the negative local maxima
    nms8, pad = s["nms"][8].reshape(-1), pl[8]["padding"]
    assert pl[8]["positives"] == 8 and (0.5, 5) in pl[8]["groups"] and len(pad) == K - 8, pl[8]
    assert (nms8 < 0).any() and (np.signbit(nms8) & (nms8 == 0)).any() and (~np.signbit(nms8) & (nms8 == 0)).any()
    assert np.all(np.diff(pad) > 0) and pad[-1] > len(pad) - 1 and (nms8[:pad[-1]] < 0).any(), pad
    rec["h_padding"] = (len(pad), int(pad[-1]))
    return rec


def require_lattice(s, plateau_tile=False):
    """a lattice scene after its upsampling: tie groups inside the top K in one tile, across tiles and tile rows, a
    tie group at the K-th place (lowest indices taken), tied plane maxima in refine; ``plateau_tile``: more than 512
    local maxima in one tile"""
    assert s["groups"] >= 10 and s["same_tile"] >= 1 and s["other_tile"] >= 1 and s["other_tile_row"] >= 1, s["groups"]
    assert len(s["straddles"]) >= 1 and all(st[4] for st in s["straddles"]), s["straddles"]
    r = s["refine"]
    assert r["max_first"] + r["max_later"] + r["max_none"] >= 1 and r["missing"] > 16, r
    if plateau_tile:
        assert s["tile_maxima"] > 512, s["tile_maxima"]
    return dict(groups=s["groups"], same_tile=s["same_tile"], other_tile_row=s["other_tile_row"],
                straddles=len(s["straddles"]), tile_maxima=s["tile_maxima"], people=s["people"],
                tied_maxima=(r["max_first"], r["max_later"], r["max_none"]))
