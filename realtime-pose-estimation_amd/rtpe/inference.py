"""Multi-scale / flip test inference.

The reference's upstream-faithful validation scripts (``legacy/valid_ae1dim.py:166-207``, ``legacy/valid_ae_avg.py``)
call ``get_multi_stage_outputs`` and ``aggregate_results`` of the upstream HigherHRNet code base
(``lib/core/inference.py`` of HRNet/HigherHRNet-Human-Pose-Estimation).  That module is NOT in the reference
repository; its published algorithm is restated here behind the same two function names, with the ``cfg`` object
replaced by keyword arguments that carry the ``cfg.TEST.* / cfg.DATASET.* / cfg.LOSS.*`` fields it reads.  All tensor
arithmetic runs in one HIP kernel (``rtpe_resize_combine``: ``dst = [dst +] resize(flip(src[:, perm])) [/ div]``,
bit-equal to ``F.interpolate(mode="bilinear", align_corners=False)`` / ``torch.flip`` / index / add / divide on the
CPU); PyTorch only allocates.  ``multi_scale_inference`` is the per-image body of valid_ae1dim.py:166-207 on top of
the accelerated teacher, warp and decode of this package.
"""
import ctypes

import torch

from . import _native as nat

# upstream dataset/transforms FLIP_CONFIG["COCO"]: left <-> right joints
FLIP_CONFIG = {"COCO": [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15],
               "COCO_WITH_CENTER": [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15, 17]}


def resize_combine(src, size, channels=None, flip=False, out=None, accumulate=False, div=1.0):
    """``out = [out +] interpolate(flip(src[:, channels]), size, bilinear, align_corners=False) [/ div]`` in one
    pass.  src (N,C,h,w) float32 on the GPU; ``channels``: list of source channels (default all); ``flip``:
    ``torch.flip(., [3])`` AFTER the resize (upstream order).  Returns ``out`` (allocated when None)."""
    nat.require_gpu(src, "resize_combine")
    if src.dtype != torch.float32 or src.dim() != 4:
        raise TypeError("resize_combine expects a float32 (N,C,h,w) tensor")
    src = src.contiguous()
    N, C, h, w = src.shape
    chans = list(range(C)) if channels is None else [int(c) for c in channels]
    oh, ow = int(size[0]), int(size[1])
    if out is None:
        if accumulate:
            raise ValueError("resize_combine: accumulate needs an existing output")
        out = torch.empty((N, len(chans), oh, ow), dtype=torch.float32, device=src.device)
    if tuple(out.shape) != (N, len(chans), oh, ow) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("resize_combine: output must be a contiguous float32 %s tensor" % ((N, len(chans), oh, ow),))
    nat.same_device("resize_combine", src, out)
    cmap = (ctypes.c_int32 * len(chans))(*chans)
    with nat.on_device(src):
        nat.check(nat.lib().rtpe_resize_combine(
            ctypes.c_void_p(src.data_ptr()), N, C, h, w, cmap, len(chans), int(bool(flip)),
            ctypes.c_void_p(out.data_ptr()), oh, ow, int(bool(accumulate)), float(div), nat.stream_ptr(src.device)))
    return out


def channel_mean(t):
    """``t.mean(dim=1)`` of a float32 (N,C,h,w) GPU tensor -> (N,h,w), bit-equal to PyTorch-CPU's op in its
    vectorised order (channels in blocks of 16, one true division) for every pixel: the tag map of the averaged-tag
    test.  One HIP kernel (csrc/tag_mean.hip); a channel slice is read where it is.  C <= 272: beyond that the CPU op
    takes an order that is not pinned, and the call is a ValueError."""
    from .third_party.group import channel_mean as op
    return op(t)


def get_multi_stage_outputs(model, image, with_flip=False, project2image=False, size_projected=None,
                            num_joints=17, with_heatmaps=(True, True), with_heatmaps_loss=(True, True),
                            with_ae=(True, False), with_ae_loss=(True, False), tag_per_joint=True,
                            flip_index=None):
    """upstream ``get_multi_stage_outputs(cfg, model, image, with_flip, project2image, size_projected)``:
    ``model(image) -> [preds (N,34,h/4,w/4), refined (N,17,h/2,w/2)]``; every output but the last is resized to the
    last one's size (bilinear, align_corners=False); the heat maps of all stages are averaged, the tag channels
    collected; with ``with_flip`` the same for the mirrored image, mirrored back and with left / right joints
    swapped; with ``project2image`` everything is resized to ``size_projected = (w, h)``.
    Returns ``(outputs, heatmaps, tags)`` as upstream: ``heatmaps`` = [avg] or [avg, avg_flipped], ``tags`` = list of
    (N,17,h,w) maps."""
    flip_index = FLIP_CONFIG["COCO"] if flip_index is None else list(flip_index)
    joints = list(range(num_joints))
    outputs = list(model(image))
    heatmaps, tags = [], []

    def stage_maps(outs, mirrored):
        size = tuple(outs[-1].shape[2:])
        n_hm = sum(1 for i in range(len(outs)) if with_heatmaps_loss[i] and with_heatmaps[i])
        avg, seen = None, 0
        for i, o in enumerate(outs):
            o = o.float()
            offset = num_joints if with_heatmaps_loss[i] else 0
            if with_heatmaps_loss[i] and with_heatmaps[i]:
                seen += 1
                src = [flip_index[j] for j in joints] if mirrored else joints
                # heatmaps_avg += output[:, :J][:, flip_index]; the division by the count rides on the last term
                avg = resize_combine(o, size, src, flip=mirrored, out=avg, accumulate=avg is not None,
                                     div=float(n_hm) if seen == n_hm else 1.0)
            if with_ae_loss[i] and with_ae[i]:
                n_tag = o.shape[1] - offset
                src = [offset + (flip_index[j] if (mirrored and tag_per_joint) else j) for j in range(n_tag)]
                tags.append(resize_combine(o, size, src, flip=mirrored))
        if avg is not None:
            heatmaps.append(avg)

    stage_maps(outputs, False)
    if with_flip:
        outputs_flip = list(model(torch.flip(image, [3])))
        stage_maps(outputs_flip, True)
        outputs = outputs + outputs_flip        # upstream appends the mirrored-back outputs; callers ignore them
    if project2image and size_projected:
        size = (int(size_projected[1]), int(size_projected[0]))
        heatmaps = [resize_combine(h, size) for h in heatmaps]
        tags = [resize_combine(t, size) for t in tags]
    return outputs, heatmaps, tags


def aggregate_results(scale_factor, final_heatmaps, tags_list, heatmaps, tags, scale_factors=(1,),
                      flip_test=True, project2image=True):
    """upstream ``aggregate_results(cfg, scale_factor, final_heatmaps, tags_list, heatmaps, tags)``: tags are kept
    for scale 1 only, the (flip-averaged) heat maps of every scale are summed at the size of the first scale"""
    if scale_factor == 1 or len(scale_factors) == 1:
        if final_heatmaps is not None and not project2image:
            tags = [resize_combine(t, final_heatmaps.shape[2:]) for t in tags]
        for t in tags:
            tags_list.append(t.unsqueeze(4))
    if flip_test:
        avg = resize_combine(heatmaps[0], heatmaps[0].shape[2:])                       # a copy
        avg = resize_combine(heatmaps[1], avg.shape[2:], out=avg, accumulate=True, div=2.0)
    else:
        avg = heatmaps[0]
    if final_heatmaps is None:
        final_heatmaps = avg
    else:       # `+=` (PROJECT2IMAGE: same size) or `+= interpolate(avg, size of final)`: the same kernel call
        resize_combine(avg, final_heatmaps.shape[2:], out=final_heatmaps, accumulate=True)
    return final_heatmaps, tags_list


def multi_scale_inference(model, parser, image, input_size=640, scale_factors=(1,), flip_test=True,
                          project2image=True, adjust=True, refine=True, device="cuda", ags=False, **stage_kw):
    """The per-image body of legacy/valid_ae1dim.py:166-207: for every test scale (largest first) warp the image,
    run the teacher (and its mirror image), aggregate; average the heat maps over the scales, concatenate the tag
    maps, group with ``parser.parse`` and map the keypoints back to image coordinates with ``get_final_preds``.
    image: (h, w, 3) uint8.  Returns ``(final_results, scores, final_heatmaps, tags)``.

    ``ags=True`` takes the branch the reference script actually runs (valid_ae1dim.py:177, :191-199, ``AGS = True``):
    the grouping sees ONE tag map for all joints - channel 0 of the first (un-mirrored) tag map of the LAST scale of
    the loop, a (1,1,h,w,1) tensor - with ``parser.tag_per_joint = False`` (the script sets the attribute on the
    caller's parser and leaves it set; so does this) and ``adjust = refine = True`` whatever the arguments say.
    ``tags`` in the result is then that tensor.

    ``ags="mean"`` (``"first"`` is ``True``; any other string is a ValueError) is the per-image body of
    legacy/valid_ae_avg.py:189-195 instead: the ONE tag map is ``tags[0].mean(dim=1)`` of the last scale of the loop -
    ``channel_mean``, PyTorch-CPU's float order - and otherwise everything is as with ``ags=True``."""
    from .third_party import transforms
    from .third_party.group import ags_mode
    ags = ags_mode(ags, "multi_scale_inference")                        # (before any GPU work)
    scale_factors = list(scale_factors)
    base_size, center, scale = transforms.get_multi_scale_size(image, input_size, 1.0, min(scale_factors))
    final_heatmaps, tags_list = None, []
    with torch.no_grad():
        for s in sorted(scale_factors, reverse=True):
            t, center, scale = transforms.warp_normalize(image, input_size, s, min(scale_factors), device=device)
            _, heatmaps, tags = get_multi_stage_outputs(model, t, flip_test, project2image, base_size, **stage_kw)
            ags_map = tags[0] if ags == "mean" else tags[0][:, 0].unsqueeze(-1).unsqueeze(0)    # valid_ae1dim.py:177
            final_heatmaps, tags_list = aggregate_results(s, final_heatmaps, tags_list, heatmaps, tags, scale_factors,
                                                          flip_test, project2image)
        if len(scale_factors) != 1:
            final_heatmaps = resize_combine(final_heatmaps, final_heatmaps.shape[2:], div=float(len(scale_factors)))
        tags = torch.cat(tags_list, dim=4)
        if ags:
            parser.tag_per_joint = False                                # valid_ae1dim.py:196
            if ags == "mean":                                           # valid_ae_avg.py:189-195, the last scale's maps
                ags_map = channel_mean(ags_map).unsqueeze(-1).unsqueeze(0)
            tags = ags_map.contiguous()
            grouped, scores = parser.parse(final_heatmaps, tags, True, True)
        else:
            grouped, scores = parser.parse(final_heatmaps, tags, adjust, refine)
    final_results = transforms.get_final_preds(grouped, center, scale,
                                               [final_heatmaps.size(3), final_heatmaps.size(2)])
    return final_results, scores, final_heatmaps, tags


def group_by_input_size(sizes):
    """``sizes``: the network input size of every image (anything hashable, e.g. the ``(w, h)`` that
    ``transforms.get_multi_scale_size`` returns) -> ``[(size, [indices])]``: one group per distinct size, groups in
    the order their first image appears, indices ascending within a group.  Pure host function."""
    groups = {}
    for i, s in enumerate(sizes):
        groups.setdefault(s, []).append(i)
    return list(groups.items())


def _match_kw(match_on):
    """the ``match_on`` keyword of ``TeacherPipeline``, checked before any GPU work; absent when None"""
    if match_on not in (None, "host", "device"):
        raise ValueError("match_on must be None, 'host' or 'device', not %r" % (match_on,))
    return {} if match_on is None else {"match_on": match_on}


def _warp_mode(warp):
    """the ``warp`` keyword of the batched drivers, checked before any GPU work: True for ``"batch"``"""
    if warp not in ("image", "batch"):
        raise ValueError("warp must be 'image' or 'batch', not %r" % (warp,))
    return warp == "batch"


def _record_ids(who, image_ids, n_images, parser, match_on):
    """``image_ids`` of the batched drivers, checked before any GPU work: None, or one id per image as a list of
    ints (``group.check_record_ids``, the rule the parser applies to every batch).  The records are written behind the
    device grouping, so ``match_on`` (or, with None, the parser as it is) must say "device": it is never switched
    silently."""
    from .third_party.group import check_record_ids
    if image_ids is None:
        return None
    if (parser.match_on if match_on is None else match_on) != "device":
        raise ValueError("%s: image_ids asks for the device-resident records, which need match_on='device'" % who)
    return check_record_ids(image_ids, n_images, who)


def _in_input_order(recs, order, n_images, device):
    """the record tensors of the batches, concatenated and put into input order: ``order[r]`` is the image of row r"""
    from .engine import RECORD_FLOATS
    if not recs:
        return torch.zeros((0, RECORD_FLOATS), dtype=torch.float32, device=device)
    rec = torch.cat(recs)
    if order == list(range(n_images)):
        return rec
    inv = [0] * n_images
    for r, i in enumerate(order):
        inv[i] = r
    # (a pinned block of the caching host allocator and an asynchronous upload: the host does not wait here either)
    inv = torch.tensor(inv, dtype=torch.int64).pin_memory() if rec.is_cuda else torch.tensor(inv, dtype=torch.int64)
    return rec.index_select(0, inv.to(rec.device, non_blocking=True))


def _stream_by_size(pipe, images, input_size, sizes, base, batch_size, warp_chunk, batch_scales=None, image_ids=None,
                    project2image=True):
    """the tail of the batched drivers: images of one ``sizes`` entry form a group (``entry[base]`` is its
    projection size ``(w, h)``), a group is cut into chunks of ``batch_size``, ``warp_chunk(warp)`` makes one item of
    ``pipe.stream`` from ``warp(s, lo)`` - the chunk's images warped at scale ``s`` as one tensor - and the keypoints
    are mapped back with the centre / scale the LAST warp of an image left.  Warps as lazily as the pipeline asks.
    ``batch_scales`` (``warp="batch"``): every ``(s, lo)`` that ``warp_chunk`` asks for, in its order; a chunk is then
    made by ONE ``transforms.warp_normalize_batch`` call for all of them, and ``warp`` only hands its tensors out.
    ``image_ids``: one id per image; the result is then ONE (len(images), RECORD_FLOATS) record tensor on the device in
    input order, the mapping back done by the record kernel with each image's ``transforms.final_preds_matrix``.
    ``project2image=False``: the decode grid, and the size ``get_final_preds`` takes, is the heat-map size
    ``[w2_0, h2_0]`` of the largest scale, half of ``entry[0]``."""
    from .third_party import transforms
    out = [None] * len(images)
    recs, order = [], []
    for key, idx in group_by_input_size(sizes):
        w, h = key[base] if project2image else (key[0][0] // 2, key[0][1] // 2)
        chunks = [idx[o:o + batch_size] for o in range(0, len(idx), batch_size)]
        meta = {}

        def batch(c):
            if batch_scales is not None:
                ts, centers, scale_arrays = transforms.warp_normalize_batch(
                    [images[i] for i in c], input_size, batch_scales, device=pipe.device)
                for n, i in enumerate(c):
                    meta[i] = (centers[n][-1], scale_arrays[n][-1])
                by_scale = dict(zip(batch_scales, ts))
                return warp_chunk(lambda s, lo: by_scale[(s, lo)])

            def warp(s, lo):
                ts = []
                for i in c:
                    t, center, scale = transforms.warp_normalize(images[i], input_size, s, lo, device=pipe.device)
                    ts.append(t)
                    meta[i] = (center, scale)
                return torch.cat(ts)
            return warp_chunk(warp)

        def records(k):     # asked when chunk k has been warped: the centre / scale its last warp left
            if any(i not in meta for i in chunks[k]):
                raise RuntimeError("warp_chunk must warp every image of a chunk before it returns: the record of an "
                                   "image needs the centre / scale of its last warp")
            return [image_ids[i] for i in chunks[k]], \
                [transforms.final_preds_matrix(*meta.pop(i), [w, h]) for i in chunks[k]]
        with torch.no_grad():
            if image_ids is not None:
                for c, rec in zip(chunks, pipe.stream((batch(c) for c in chunks), out_hw=(h, w), records=records)):
                    recs.append(rec)
                    order += c
                continue
            for c, res in zip(chunks, pipe.stream((batch(c) for c in chunks), out_hw=(h, w))):
                for i, (people, scores) in zip(c, res):
                    center, scale = meta.pop(i)
                    out[i] = (transforms.get_final_preds([people], center, scale, [w, h]), scores)
    if image_ids is not None:
        return _in_input_order(recs, order, len(images), pipe.device)
    return out


def flip_test_inference(model, parser, images, input_size=640, adjust=True, refine=True, batch_size=32,
                        device="cuda", ags=False, match_on=None, warp="image", image_ids=None, project2image=True):
    """Batched drop-in for ``multi_scale_inference(model, parser, img, input_size, scale_factors=(1,),
    flip_test=True, project2image=True, adjust, refine)`` over a list of (h, w, 3) uint8 images: every image is
    warped to its network input size, images of one size are batched (``batch_size`` at a time) through
    ``TeacherPipeline(flip_test=True).stream`` - both forwards on the GPU, the decode from the network outputs
    (``HeatmapParser.parse_flip``) - and the keypoints are mapped back with ``get_final_preds``.  Returns
    ``[(final_results, scores)]`` in input order, each bit-identical to the first two items the per-image call
    returns (the forward is batch-invariant).

    ``ags=True``: the drop-in for ``multi_scale_inference(model, parser, img, input_size, (1,), True, True,
    ags=True)`` instead (``multi_scale_batch_inference`` with ``scale_factors=(1,)``, see there); ``ags="mean"``
    likewise for the averaged-tag test.

    ``match_on``: passed to ``TeacherPipeline`` (``"host"`` / ``"device"``: where the candidates are grouped into
    people; None leaves the parser as it is).

    ``warp``: ``"image"`` warps one image at a time (``transforms.warp_normalize``), ``"batch"`` a whole chunk with
    one upload and one launch (``transforms.warp_normalize_batch``, needs real uint8 images); same bits.

    ``image_ids`` (one int per image; needs ``match_on="device"``, given here or set on the parser): the result is one
    ``(len(images), engine.RECORD_FLOATS)`` float32 tensor on the device in input order - ``engine.pack_records`` of
    the list result, ``get_final_preds`` included, written by the record kernel; the host reads no keypoint.

    ``project2image=False``: the drop-in for the per-image call with ``project2image=False`` instead - the decode on
    the heat-map grid (h2, w2), a quarter of the pixels and no projection (``multi_scale_batch_inference`` with
    ``scale_factors=(1,)``, see there); not with ``ags``."""
    from .engine import TeacherPipeline
    from .third_party import transforms
    from .third_party.group import ags_mode
    batched = _warp_mode(warp)
    ags = ags_mode(ags, "flip_test_inference")
    if ags or not project2image:
        return multi_scale_batch_inference(model, parser, images, input_size, (1,), True, adjust, refine, batch_size,
                                           device=device, ags=ags, warp=warp, image_ids=image_ids,
                                           project2image=project2image, **_match_kw(match_on))
    if not parser.tag_per_joint:
        raise ValueError("flip_test_inference: the flip test needs a parser with tag_per_joint=True")
    if batch_size < 1:
        raise ValueError("flip_test_inference: batch_size must be positive")
    images = list(images)
    kw = _match_kw(match_on)
    image_ids = _record_ids("flip_test_inference", image_ids, len(images), parser, match_on)
    sizes = [(transforms.get_multi_scale_size(img, input_size, 1.0, 1)[0],) for img in images]
    pipe = TeacherPipeline(model, parser, device=device, flip_test=True, **kw)
    return _stream_by_size(pipe, images, input_size, sizes, 0, batch_size, lambda warp: warp(1, 1),
                           [(1, 1)] if batched else None, image_ids)


def check_scale_factors(scale_factors):
    """the test scales of the batched multi-scale path in the loop order of ``multi_scale_inference`` (descending),
    refused unless 1 is among them, they are distinct and there are at most 4.  Pure host function."""
    scales = list(scale_factors)
    if not scales or 1 not in scales:
        raise ValueError("multi-scale test: 1 must be among the scales %s (the tags and the projection size come "
                         "from scale 1)" % (tuple(scales),))
    if len(set(float(s) for s in scales)) != len(scales):
        raise ValueError("multi-scale test: the scales %s are not distinct" % (tuple(scales),))
    if len(scales) > 4:
        raise ValueError("multi-scale test: at most 4 scales, got %d" % len(scales))
    if any(not s > 0 for s in scales):
        raise ValueError("multi-scale test: the scales %s must be positive" % (tuple(scales),))
    return tuple(sorted(scales, reverse=True))


def multi_scale_input_sizes(image, input_size, scale_factors):
    """the network input size ``(w, h)`` of ``image`` at every scale of ``scale_factors`` (descending, as
    ``check_scale_factors`` returns them), as ``warp_normalize`` makes them; refused unless every size is a multiple
    of 32 (the network's total stride).  Pure host function."""
    from .third_party import transforms
    lo = min(scale_factors)
    sizes = tuple(transforms.get_multi_scale_size(image, input_size, s, lo)[0] for s in scale_factors)
    for s, (w, h) in zip(scale_factors, sizes):
        if w % 32 or h % 32:
            raise ValueError("multi-scale test: the input size %d x %d at scale %s is not a multiple of 32"
                             % (w, h, s))
    return sizes


def multi_scale_batch_inference(model, parser, images, input_size=640, scale_factors=(2, 1, 0.5), flip_test=True,
                                adjust=True, refine=True, batch_size=32, max_forward_pixels=None, device="cuda",
                                ags=False, match_on=None, warp="image", image_ids=None, project2image=True):
    """Batched drop-in for ``multi_scale_inference(model, parser, img, input_size, scale_factors, flip_test,
    project2image=True, adjust, refine)`` over a list of (h, w, 3) uint8 images: images are grouped by their input
    sizes at every scale, every image is warped at every scale, each group is streamed ``batch_size`` images at a
    time through ``TeacherPipeline(scale_factors=...)`` - every scale's forwards in sub-batches of at most
    ``max_forward_pixels`` input pixels (default ``engine.MAX_FORWARD_PIXELS``), the decode from the network outputs
    (``HeatmapParser.parse_multi_scale``) - and the keypoints are mapped back with ``get_final_preds`` and the
    centre / scale of the smallest-scale warp (what the per-image loop's last iteration leaves).  Returns
    ``[(final_results, scores)]`` in input order, each bit-identical to the first two items the per-image call
    returns.  The scales and every input size are checked before any GPU work.

    ``ags=True``: the drop-in for the per-image call with ``ags=True``, its quirks included: the decode adjusts and
    refines whatever ``adjust`` / ``refine`` say (the pipeline always does both), and ``parser.tag_per_joint`` is set to
    False and left so (any parser is accepted); the decode is ``TeacherPipeline(..., ags=True)``.  ``ags="mean"``: the
    same for the averaged-tag test, ``multi_scale_inference(..., ags="mean")`` (``"first"`` is ``True``; any other
    string is a ValueError before any GPU work).

    ``match_on``: passed to ``TeacherPipeline`` (``"host"`` / ``"device"``; None leaves the parser as it is).

    ``warp``: ``"image"`` warps one image and one scale at a time, ``"batch"`` a whole chunk at every scale with one
    upload and one launch per scale (``transforms.warp_normalize_batch``, needs real uint8 images); same bits.

    ``image_ids``: as for ``flip_test_inference`` - one record tensor on the device in input order.

    ``project2image=False``: the drop-in for the per-image call with ``project2image=False`` - the heat maps are
    averaged at each scale's own heat-map size and summed at that of the largest scale, where the decode runs
    (``TeacherPipeline(..., project2image=False)``); ``get_final_preds``, and the ``xform`` of the records, take that
    size ``[w2_0, h2_0]``.  ``ags`` together with it is a ValueError before any GPU work."""
    from .engine import MAX_FORWARD_PIXELS, TeacherPipeline
    from .third_party.group import ags_mode
    ags = ags_mode(ags, "multi_scale_batch_inference")
    if ags and not project2image:
        raise ValueError("multi_scale_batch_inference: ags has no batched form with project2image=False (it stays "
                         "per-image, multi_scale_inference)")
    batched = _warp_mode(warp)
    kw = _match_kw(match_on)
    scales = check_scale_factors(scale_factors)
    if not ags and not parser.tag_per_joint:
        raise ValueError("multi_scale_batch_inference: needs a parser with tag_per_joint=True")
    if batch_size < 1:
        raise ValueError("multi_scale_batch_inference: batch_size must be positive")
    images = list(images)
    image_ids = _record_ids("multi_scale_batch_inference", image_ids, len(images), parser, match_on)
    sizes = [multi_scale_input_sizes(img, input_size, scales) for img in images]
    lo, base = min(scales), scales.index(1)
    if ags:
        parser.tag_per_joint = False                                    # as multi_scale_inference(..., ags=True)
    pipe = TeacherPipeline(model, parser, device=device, flip_test=flip_test, scale_factors=scales,
                           max_forward_pixels=MAX_FORWARD_PIXELS if max_forward_pixels is None else max_forward_pixels,
                           ags=ags, **({} if project2image else {"project2image": False}), **kw)
    # one tensor per scale, largest first: the last warp, whose centre / scale is kept, is the smallest scale's
    return _stream_by_size(pipe, images, input_size, sizes, base, batch_size,
                           lambda warp: [warp(s, lo) for s in scales], [(s, lo) for s in scales] if batched else None,
                           image_ids, project2image)


class _Shape:
    """what ``get_multi_scale_size`` reads of an image: its ``shape``"""

    def __init__(self, h, w):
        self.shape = (h, w, 3)


def plain_plan(shapes, input_size=640, batch_size=32, max_forward_pixels=None, by_original_size=False):
    """the batches of ``plain_inference`` for images of the given ``(h, w)`` shapes: ``[[indices]]``, images grouped
    by their network input size only (``by_original_size``: by input size AND original size - what a decode with one
    size per batch needs), every group cut into chunks of at most ``batch_size`` images and at most
    ``max_forward_pixels`` input pixels (default ``engine.MAX_FORWARD_PIXELS``).  Pure host function."""
    from .engine import MAX_FORWARD_PIXELS, forward_plan
    from .third_party import transforms
    if batch_size < 1:
        raise ValueError("plain_inference: batch_size must be positive")
    budget = int(MAX_FORWARD_PIXELS if max_forward_pixels is None else max_forward_pixels)
    keys = []
    for h, w in shapes:
        size = transforms.get_multi_scale_size(_Shape(int(h), int(w)), input_size, 1.0, 1)[0]
        keys.append((size, (int(h), int(w))) if by_original_size else (size,))
    chunks = []
    for key, idx in group_by_input_size(keys):
        w, h = key[0]
        chunks += [idx[n0:n0 + n] for n0, n in forward_plan(len(idx), (h, w), min(budget, batch_size * h * w))]
    return chunks


def plain_inference(model, parser, images, input_size=640, batch_size=32, max_forward_pixels=None, device="cuda",
                    match_on=None, warp="image", image_ids=None):
    """The batched ``validate_hhrnet.py:84-105`` over a list of (h, w, 3) uint8 images: every image is warped to its
    network input size (``warp_normalize(img, input_size, 1, 1)``), images of one INPUT size are batched whatever
    their original sizes - at most ``batch_size`` images and ``max_forward_pixels`` input pixels per forward
    (``plain_plan``) - and streamed through ``TeacherPipeline``, which decodes every image at its own original
    ``(h, w)`` (``HeatmapParser.parse_lowres`` with one size per image).  Returns ``[(people, scores)]`` in input
    order, people in the pixel coordinates of the original image, each bit-identical to the per-image loop body::

        t, _, _ = warp_normalize(img, input_size, 1, 1, device=device)
        preds, refined = model(t)
        parser.parse_lowres(refined, preds[:, 17:], img.shape[:2])[0]

    (the forward is batch-invariant).  This protocol has no ``get_final_preds`` step.  ``match_on``: passed to
    ``TeacherPipeline`` (``"host"`` / ``"device"``; None leaves the parser as it is).  The batches are planned, and
    an image beyond the pixel budget refused, before any GPU work.  ``warp``: ``"image"`` makes a batch with one
    ``warp_normalize`` call per image and a concatenation, ``"batch"`` with one ``transforms.warp_normalize_batch``
    call (one upload, one launch; needs real uint8 images); same bits.

    ``image_ids`` (one int per image; needs ``match_on="device"``, given here or set on the parser): the result is one
    ``(len(images), engine.RECORD_FLOATS)`` float32 tensor on the device in input order, ``engine.pack_records`` of the
    list result (no transform: the people are in the original image's pixel coordinates already)."""
    from .engine import TeacherPipeline
    from .third_party import transforms
    kw = _match_kw(match_on)
    batched = _warp_mode(warp)
    images = list(images)
    image_ids = _record_ids("plain_inference", image_ids, len(images), parser, match_on)
    shapes = [tuple(int(v) for v in img.shape[:2]) for img in images]
    chunks = plain_plan(shapes, input_size, batch_size, max_forward_pixels)
    out = [None] * len(images)
    if not chunks:
        return out if image_ids is None else _in_input_order([], [], 0, device)
    pipe = TeacherPipeline(model, parser, device=device, **kw)

    def batch(c):
        if batched:
            return transforms.warp_normalize_batch([images[i] for i in c], input_size, ((1, 1),),
                                                   device=pipe.device)[0][0]
        return torch.cat([transforms.warp_normalize(images[i], input_size, 1, 1, device=pipe.device)[0] for i in c])
    with torch.no_grad():
        if image_ids is not None:
            recs = list(pipe.stream((batch(c) for c in chunks), out_hw=lambda k: [shapes[i] for i in chunks[k]],
                                    records=lambda k: ([image_ids[i] for i in chunks[k]], None)))
            return _in_input_order(recs, [i for c in chunks for i in c], len(images), pipe.device)
        results = pipe.stream((batch(c) for c in chunks), out_hw=lambda k: [shapes[i] for i in chunks[k]])
        for c, res in zip(chunks, results):
            for i, r in zip(c, res):
                out[i] = r
    return out
