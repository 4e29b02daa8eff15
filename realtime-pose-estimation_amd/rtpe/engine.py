"""Inference loops of the hot path.

``eval_student`` keeps the name and signature of the reference's
``rtpe/engine.py:21-75``.  ``TeacherPipeline`` is the accelerated body of the
per-image loops of ``validate_hhrnet.py:84-105`` / ``teacher_inference.py:67-90``:
batched forward on the HIP executor + fused decode, one process per GPU, with
the weights broadcast and the keypoints all-gathered over RCCL when a process
group is active.
"""
from collections import OrderedDict

import numpy as np
import torch

from .third_party.group import HeatmapParser, per_image_sizes

HM_PARSER_PARAMS = {"max_num_people": 30, "detection_threshold": 0.1, "tag_threshold": 1.0,
                    "use_detection_val": True, "ignore_too_much": False, "tag_per_joint": True,
                    "nms_ksize": 5, "nms_padding": 2}       # validate_hhrnet.py:40-47
NUM_HEATMAPS = 17
MAX_PEOPLE_RECORD = 30
RECORD_FLOATS = 2 + MAX_PEOPLE_RECORD + MAX_PEOPLE_RECORD * NUM_HEATMAPS * 4   # 8,288 B
# the most input pixels one forward of the multi-scale pipeline takes: the bench shape (32 x 640 x 640), i.e. tensors
# and workspaces no larger than those the plain pipeline uses (several kernels index with 32 bits)
MAX_FORWARD_PIXELS = 32 * 640 * 640


def forward_plan(n, hw, max_forward_pixels=MAX_FORWARD_PIXELS):
    """sub-batches ``[(n0, count)]`` of a batch of n images of input size hw = (H, W) such that no forward has more
    than ``max_forward_pixels`` input pixels (per image: H * W).  Pure host function."""
    per = int(max_forward_pixels) // (int(hw[0]) * int(hw[1]))
    if per < 1:
        raise ValueError("an input of %d x %d pixels exceeds the forward pixel budget of %d"
                         % (hw[0], hw[1], max_forward_pixels))
    return [(o, min(per, n - o)) for o in range(0, n, per)]


def eval_student(model, hm_parser, val_dataloader, device,
                 plot_every=None, save_every=None, save_dir="/tmp"):
    """reference engine.py:21-75: run ``model`` over the loader, decode with
    ``hm_parser.parse`` and return the dataset's evaluation dict.

    Each batch is a tuple whose first two items are ``(img_id, img)``.  ``model``
    may return one tensor (heatmaps in channels [:17], tags in [17:], as the
    reference's students did), the teacher's ``[preds, refined]`` list, or the
    dual-head student's ``(att, det)`` tuple (config 5).
    Plotting / image saving (``plot_every`` / ``save_every``) are not part of
    the accelerated path and are ignored.
    """
    model.eval()
    all_preds, all_scores = [], []
    for batch_i, batch in enumerate(val_dataloader):
        img = batch[1]
        out_hw = tuple(img.shape[2:])
        img = img.to(device)
        with torch.no_grad():
            try:
                pred = model(img, out_hw)
            except TypeError:
                pred = model(img)
        if isinstance(pred, (list, tuple)) and pred[0].shape[1] == 1:
            # dual-head student (rtpe/students.py:724-771): (attention mask, det) with the heat maps in
            # det[:, :17] and the tags in det[:, 17:18], both at 1/4 resolution; decoded like the teacher's
            # maps (validate_hhrnet.py:93-101): bilinear to the image size, then parse
            det = pred[1].float()
            res = hm_parser.parse_lowres(det[:, :NUM_HEATMAPS].contiguous(), det[:, NUM_HEATMAPS:NUM_HEATMAPS + 1]
                                         .expand(-1, NUM_HEATMAPS, -1, -1).contiguous(), out_hw)
            grouped, scores = [res[0][0]], res[0][1]
        elif isinstance(pred, (list, tuple)):
            preds, refined = pred
            res = hm_parser.parse_lowres(refined.float(), preds[:, NUM_HEATMAPS:].float(), out_hw)
            grouped, scores = [res[0][0]], res[0][1]
        else:
            pred = pred.detach().float()
            grouped, scores = hm_parser.parse(pred[:, :NUM_HEATMAPS], pred[:, NUM_HEATMAPS:].unsqueeze(-1),
                                              adjust=True, refine=True)
        all_preds.append([x for x in grouped[0] if x.size > 0])
        all_scores.append(scores)
    dataset = getattr(val_dataloader, "dataset", None)
    if dataset is not None and hasattr(dataset, "evaluate"):
        eval_dict, _ = dataset.evaluate(all_preds, all_scores, ".", False, False)
        return eval_dict
    return OrderedDict(images=len(all_preds), people=sum(len(p) for p in all_preds))


_PIN_RING = {}


def pack_records(image_ids, results, device):
    """fixed-size keypoint records for the all-gather: per image
    ``[image_index, n_people, scores[30], kpts[30][17][4]]`` as float32 (image ids are exact up to 2^24;
    COCO's largest is 581,929).  On a GPU the records go
    through a small ring of pinned host buffers and an asynchronous copy, so packing never waits
    for the kernels queued on the stream."""
    device = torch.device(device)
    n_img = len(results)
    if device.type == "cuda":
        ring = _PIN_RING.setdefault(n_img, {"i": 0, "bufs": []})
        if len(ring["bufs"]) < 4:
            ring["bufs"].append(torch.zeros((n_img, RECORD_FLOATS), dtype=torch.float32, pin_memory=True))
        host = ring["bufs"][ring["i"] % len(ring["bufs"])]
        ring["i"] += 1
        host.zero_()
        rec = host.numpy()
    else:
        host = None
        rec = np.zeros((n_img, RECORD_FLOATS), np.float32)
    for i, (img_id, (people, scores)) in enumerate(zip(image_ids, results)):
        n = min(len(people) if people.ndim == 3 else 0, MAX_PEOPLE_RECORD)
        rec[i, 0], rec[i, 1] = img_id, n
        if n:
            rec[i, 2:2 + n] = np.asarray(scores[:n], np.float32)
            rec[i, 2 + MAX_PEOPLE_RECORD:2 + MAX_PEOPLE_RECORD + n * NUM_HEATMAPS * 4] = \
                people[:n, :, :4].reshape(-1)
    if host is not None:
        return host.to(device, non_blocking=True)
    return torch.from_numpy(rec).to(device)


def unpack_records(rec):
    out = {}
    for r in rec.cpu().numpy():
        n = int(r[1])
        kp = r[2 + MAX_PEOPLE_RECORD:2 + MAX_PEOPLE_RECORD + n * NUM_HEATMAPS * 4]
        out[int(r[0])] = (kp.reshape(n, NUM_HEATMAPS, 4).copy(), r[2:2 + n].copy())
    return out


class _Kind:
    """One kind of batch: everything of a pipeline that depends on the test protocol, as the five steps that the loop
    (``TeacherPipeline._stream_loop``) and the synchronous call (``TeacherPipeline._run``) take in this order.

    ``begin(k, batch) -> (batch, hw)``: every host check of the batch and of its decode size(s), before any GPU work;
    the batch as the forwards take it and the decode size resolved (default: the input size of the first tensor).
    ``tensors(batch)``: the input tensors of the batch, first the one whose ``shape[0]`` counts the images.
    ``open(batch, hw, decode) -> state | None``: what the decode needs before the forwards, through ``decode``.
    ``forwards(k, batch, on_forward, state, decode) -> outs``: the forwards on the current stream -> the tuple of FRESH
    output tensors the top-k reads.  ``topk(outs, hw, state) -> st``: phase 1 of the decode (on the decode stream) ->
    the state that ``lowres_match`` / ``lowres_finish`` take.
    ``decode(fn, *args, after=None, uses=())`` calls ``fn(*args)`` on the decode stream, behind the event ``after``,
    with the tensors ``uses`` kept for that stream.  ``out_hw_of(k)``: the ``out_hw`` of batch k as the caller gave it."""

    def __init__(self, pipe, out_hw_of=None):
        self.pipe, self.out_hw_of = pipe, out_hw_of

    def begin(self, k, batch):
        hw = self.pipe._decode_hw(self.out_hw_of(k), batch)
        return batch, hw if hw is not None else tuple(self.tensors(batch)[0].shape[2:])

    def tensors(self, batch):
        return [batch]

    def open(self, batch, hw, decode):
        return None


class _TeacherPlain(_Kind):
    """a (N,3,H,W) tensor through the teacher: one forward and ``lowres_topk``, or with ``flip_test`` the forwards of
    the batch and of its mirror image (made and read on the same stream) and ``flip_topk`` of the pair;
    ``on_forward(k, x)`` replaces each forward"""

    def forwards(self, k, x, on_forward, state, decode):
        p = self.pipe
        fwd = on_forward if on_forward is not None else (lambda _k, t: p.model(t))
        preds, refined = fwd(k, x)
        if not p.flip_test:
            return preds, refined
        preds_f, refined_f = fwd(k, p.mirror(x))
        return preds, refined, preds_f, refined_f

    def topk(self, outs, hw, state):
        p = self.pipe
        if p.flip_test:
            return p.parser.flip_topk(*outs, hw, p.flip_index)
        preds, refined = outs
        return p.parser.lowres_topk(refined, preds[:, NUM_HEATMAPS:], hw)


class _TeacherMultiScale(_Kind):
    """one (N,3,H_i,W_i) tensor per scale through the teacher (``scale_factors``): ``open`` makes the maps buffer
    (``ms_begin``), every sub-batch of every scale (``forward_plan``) is forwarded [with its mirror image] and prepared
    on the decode stream behind an event of its own (``ms_prep``), the top-k is ``ms_topk``; ``on_forward(k, x)``
    replaces each sub-batch's forward.  The check of the per-scale inputs and the default decode size (the scale-1
    input size) sit in ``open``, behind the check of the records, where callers have always met them."""

    def begin(self, k, batch):
        return batch, self.pipe._decode_hw(self.out_hw_of(k), batch)

    def tensors(self, batch):
        return list(batch) if isinstance(batch, (list, tuple)) else [batch]

    def open(self, xs, out_hw, decode):
        p = self.pipe
        if not isinstance(xs, (list, tuple)) or len(xs) != len(p.scale_factors):
            raise ValueError("TeacherPipeline: the multi-scale pipeline takes one input tensor per scale (%d)"
                             % len(p.scale_factors))
        for x in xs:
            if x.dim() != 4 or x.shape[0] != xs[0].shape[0]:
                raise ValueError("TeacherPipeline: the inputs of the scales must be (N,3,H,W) with the same N")
        if out_hw is None and p.project2image:  # (without projection the parser takes the refined size of the largest)
            out_hw = tuple(xs[p.scale_factors.index(1)].shape[2:])
        return decode(p.parser.ms_begin, xs[0].shape[0], [(x.shape[2] // 2, x.shape[3] // 2) for x in xs], out_hw,
                      p.scale_factors, p.flip_test, p.flip_index, p.device, p.ags, p.project2image)

    def forwards(self, k, xs, on_forward, st, decode):
        p = self.pipe
        fwd = (lambda t: on_forward(k, t)) if on_forward is not None else p.model
        for i, x in enumerate(xs):
            for n0, n in forward_plan(x.shape[0], x.shape[2:], p.max_forward_pixels):
                xb = x[n0:n0 + n]
                outs = tuple(fwd(xb))
                if p.flip_test:
                    outs = outs + tuple(fwd(p.mirror(xb)))
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(p.device))
                decode(p.parser.ms_prep, st, i, outs, n0, after=ev, uses=outs)
        return ()                               # (the network outputs are consumed)

    def topk(self, outs, hw, st):
        return self.pipe.parser.ms_topk(st)


class _StudentPlain(_Kind):
    """a tensor ``x`` or a pair ``(x, alt)`` through a dual-head student: ``model(x[, alt=alt])`` and
    ``lowres_topk_shared`` straight from ``det``; ``on_forward(k, batch)`` gets the batch as it was given"""

    def tensors(self, batch):
        return [batch] if torch.is_tensor(batch) else [t for t in batch if torch.is_tensor(t)]

    def forwards(self, k, batch, on_forward, state, decode):
        if on_forward is not None:
            att, det = on_forward(k, batch)
            return att, det
        x, alt = (batch, None) if torch.is_tensor(batch) else batch
        return self.pipe._att_det(self.pipe.model(x) if alt is None else self.pipe.model(x, alt=alt))

    def topk(self, outs, hw, state):
        det = outs[1].float()
        J = det.shape[1] - 1
        return self.pipe.parser.lowres_topk_shared(det[:, :J], det[:, J:], hw)


class _StudentMixed(_StudentPlain):
    """a mixed-size batch through a student's ``forward_mixed``: ``hw`` is the list of the images' sizes and the top-k
    ``lowres_topk_mixed`` on the ``det`` canvas.  ``packed``: the batch is the ``(canvas, sizes[, alt_canvas])`` that
    ``call_mixed`` / ``call_frames`` have packed and checked themselves"""

    def __init__(self, pipe, packed=False):
        self.pipe, self.packed = pipe, packed

    def begin(self, k, batch):
        return (batch, batch[1]) if self.packed else self.pipe._mixed_begin(batch)

    def forwards(self, k, batch, on_forward, state, decode):
        return self.pipe._mixed_forwards(k, batch, on_forward)

    def topk(self, outs, sizes, state):
        return self.pipe.parser.lowres_topk_mixed(outs[1].float(), sizes)


class TeacherPipeline:
    """forward + decode for batches of pre-processed images on one GPU.

    ``flip_test=True``: the upstream single-scale + flip test protocol (rtpe/inference.py ``multi_scale_inference``
    with ``scale_factors=(1,), flip_test=True, project2image=True``) for whole batches: every batch is mirrored on
    the GPU, both forwards run and ``HeatmapParser.parse_flip`` decodes the pair (``flip_index``: the joint
    permutation, default ``FLIP_CONFIG["COCO"]``).  People then carry 5 columns (x, y, val, tag of the image, tag of
    the mirror image) in input-pixel coordinates of the projection size; ``gather`` / ``pack_records`` keep the
    first 4, i.e. the mirror image's tag is dropped from the records.

    ``scale_factors`` (a tuple containing 1, at most 4 distinct scales; None: a single scale, as above): the upstream
    multi-scale test protocol (``multi_scale_inference(..., scale_factors, flip_test, project2image=True)``).
    ``__call__`` and ``stream()`` then take one input tensor per scale - the same images warped at every scale - in
    descending scale order, run every scale's forward(s) in sub-batches of at most ``max_forward_pixels`` input
    pixels (``forward_plan``; the forward is batch-invariant, so the bits do not depend on it) and decode with
    ``HeatmapParser.parse_multi_scale`` at the scale-1 input size.  People carry 4 + flip_test columns.

    ``ags=True`` (needs ``scale_factors``; ``(1,)`` for the single-scale protocol): the AGS branch of
    ``multi_scale_inference(..., ags=True)`` - one tag map per image, channel 0 of the un-mirrored tag maps of the
    smallest scale, shared by all joints; any parser is accepted (its ``tag_per_joint`` is not read).  People carry 4
    columns, with or without flip.  ``ags="mean"``: the averaged-tag test instead - that one tag map is the mean of
    the joints' tag maps (``HeatmapParser.parse_multi_scale``); ``"first"`` is ``True``, any other string a ValueError.

    ``project2image=False`` (needs ``scale_factors``; ``(1,)`` for the single-scale protocol; not with ``ags``): the
    test without projection to the image, ``multi_scale_inference(..., project2image=False)`` - the decode runs on the
    refined size of the largest scale's input, r_0 = (H_0 / 2, W_0 / 2) (``HeatmapParser.parse_multi_scale``); people
    are in heat-map pixels of that grid, and ``out_hw`` must be None or r_0.

    ``match_on``: ``"host"`` / ``"device"`` sets the parser's ``match_on`` (where the candidates are grouped into
    people, ``HeatmapParser``); None leaves the parser as it is.  With ``"device"`` the ``lowres_match`` call of
    ``stream()`` blocks on nothing; the order of the loop and the two-step delay of the results stay.

    Device-resident records (``match_on="device"`` only): ``__call__(..., image_ids=...)`` and ``stream(records=...)``
    return, per batch, the (N, RECORD_FLOATS) float32 tensor that ``pack_records`` would build from the list result -
    written by a kernel behind adjust + refine (``HeatmapParser.lowres_match``), never read by the host; ``gather``
    takes it as it is.  ``xform`` (N, 6): per image the float64 matrix of ``transforms.final_preds_matrix``, applied
    to (x, y) as ``get_final_preds`` does.

    All of this that depends on the protocol is a kind of batch (``_Kind``; ``_kind`` chooses it).  ``__call__`` is the
    synchronous runner ``_run`` and ``stream()`` the loop ``_stream_loop`` on that kind; neither knows a protocol."""

    project2image = True    # (the default of every pipeline; an instance asked for the other protocol sets its own)

    def __init__(self, model, parser=None, device=None, flip_test=False, flip_index=None, scale_factors=None,
                 max_forward_pixels=MAX_FORWARD_PIXELS, ags=False, match_on=None, project2image=True):
        from .third_party.group import ags_mode
        ags = ags_mode(ags, "TeacherPipeline")  # False, True or "mean" (before any GPU work)
        self.project2image = bool(project2image)
        if not self.project2image and scale_factors is None:
            raise ValueError("TeacherPipeline: project2image=False needs scale_factors (use (1,) for the single-scale "
                             "protocol)")
        if not self.project2image and ags:
            raise ValueError("TeacherPipeline: ags has no batched form with project2image=False")
        if ags and scale_factors is None:
            raise ValueError("TeacherPipeline: ags=True needs scale_factors (use (1,) for the single-scale protocol)")
        if match_on not in (None, "host", "device"):
            raise ValueError("TeacherPipeline: match_on must be None, 'host' or 'device', not %r" % (match_on,))
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.model = model.to(self.device).eval()
        self.parser = parser or HeatmapParser(num_joints=NUM_HEATMAPS, **HM_PARSER_PARAMS)
        if match_on is not None:                # None: the parser as it is
            self.parser.match_on = match_on
        self.flip_test = bool(flip_test)
        self.flip_index = None if flip_index is None else [int(q) for q in flip_index]
        self.ags = ags
        if self.flip_test and not self.parser.tag_per_joint and not self.ags:
            raise ValueError("TeacherPipeline: the flip test needs a parser with tag_per_joint=True")
        self.scale_factors = None
        self.max_forward_pixels = int(max_forward_pixels)
        if scale_factors is not None:
            from .inference import check_scale_factors
            self.scale_factors = check_scale_factors(scale_factors)
            if not self.parser.tag_per_joint and not self.ags:
                raise ValueError("TeacherPipeline: the multi-scale test needs a parser with tag_per_joint=True")

    def _kind(self, out_hw_of):
        """the kind of this pipeline's batches (``_Kind``): the ONE place where the protocol switches choose - the flip
        test is a switch inside the plain kind.  ``out_hw_of(k)``: the ``out_hw`` of batch k as the caller gave it"""
        return (_TeacherMultiScale if self.scale_factors is not None else _TeacherPlain)(self, out_hw_of)

    def _decode_hw(self, out_hw, images):
        """``out_hw`` of one batch, checked before any GPU work: None, ``(h, w)`` or one ``(h, w)`` per image - the
        plain protocol only: the flip and multi-scale tests decode at the projection size, one per batch"""
        if out_hw is None:
            return None
        x0 = images[0] if isinstance(images, (list, tuple)) else images
        sizes = per_image_sizes(out_hw, x0.shape[0], "TeacherPipeline")
        if sizes is None:
            if not self.project2image:
                r0 = (x0.shape[2] // 2, x0.shape[3] // 2)
                if (int(out_hw[0]), int(out_hw[1])) != r0:
                    raise ValueError("TeacherPipeline: without projection the decode grid is the refined size %s of "
                                     "the largest scale, not out_hw = %s" % (r0, tuple(out_hw)))
            return tuple(out_hw)
        if self.flip_test or self.scale_factors is not None:
            raise ValueError("TeacherPipeline: per-image decode sizes are for the plain protocol only; with flip_test "
                             "or scale_factors the decode size is the projection size of the batch")
        return sizes

    @torch.no_grad()
    def forward(self, images):
        return self.model(images)

    @staticmethod
    def mirror(images):
        """``torch.flip(images, [3])`` with the resize_combine kernel (an identity resize of the mirrored planes)"""
        from .inference import resize_combine
        return resize_combine(images, images.shape[2:], flip=True)

    def _records(self, x, image_ids, xform):
        """the ``records`` argument of the parser for one batch, checked before any GPU work; None without ids.
        ``x``: the tensor whose ``shape[0]`` counts the images (``_Kind.tensors``)"""
        if image_ids is None:
            if xform is not None:
                raise ValueError("TeacherPipeline: xform goes with image_ids (the device-resident records)")
            return None
        return self.parser.check_records(x.shape[0], (image_ids, xform))

    @torch.no_grad()
    def _run(self, kind, batch, image_ids=None, xform=None):
        """one batch of any kind, start to finish on the current stream: the synchronous call of every pipeline.  The
        steps of the kind in the order of the loop, each decode step called where it is asked for."""
        def decode(fn, *args, after=None, uses=()):
            return fn(*args)
        batch, hw = kind.begin(0, batch)
        records = self._records(kind.tensors(batch)[0], image_ids, xform)
        state = kind.open(batch, hw, decode)
        outs = kind.forwards(0, batch, None, state, decode)
        st = kind.topk(outs, hw, state)
        self.parser.lowres_match(st, records=records)
        return self.parser.lowres_finish(st)

    def __call__(self, images, out_hw=None, image_ids=None, xform=None):
        """images (N,3,H,W) on the GPU -> list of (people, scores) per image;
        out_hw = decode resolution (original image size), default (H, W) - one ``(h, w)`` for the batch or a sequence
        of N pairs, one per image (``HeatmapParser.parse_lowres``); with ``flip_test`` the projection size.
        With ``scale_factors``: images = one tensor per scale (descending), out_hw default = the scale-1 (H, W).
        With ``image_ids`` (N ints; ``match_on="device"``) [and ``xform`` (N, 6) float64]: the (N, RECORD_FLOATS)
        record tensor on the device instead of the lists (class docstring)."""
        return self._run(self._kind(lambda k: out_hw), images, image_ids, xform)

    def stream(self, batches, out_hw=None, on_forward=None, decode_stream=None, in_flight=None, exclusive=None,
               records=None):
        """Software-pipelined loop over an iterable of (N,3,H,W) GPU batches, in the order
        F(k) R(k-1) T(k)  (forward, adjust+refine of the previous batch, fused top-k).  The host part
        of the decode of batch k-1 (tag matching on the host cores) runs while the GPU executes F(k),
        whose launches are already queued; the GPU never waits for the host.  The decode tables travel
        through pinned host memory that the kernels read and write in place (no copy commands in the
        stream).

        ``decode_stream``: ``None`` (default) = environment ``RTPE_DECODE_STREAM`` (default "side");
        ``"side"`` puts R and T on a second HIP stream that waits for F(k) by event: the
        network's ~330 kernels per forward leave the chip partly idle at every kernel boundary (a
        persistent one-workgroup-per-CU kernel ends with its slowest workgroup), and the decode's many
        small workgroups fill those gaps instead of costing their own ~0.9 ms of stream time;
        ``"same"`` keeps everything on the current stream.

        ``in_flight`` (default: environment ``RTPE_FORWARDS_IN_FLIGHT``, default 2): forwards of consecutive batches
        alternate between that many internal HIP streams, each with an activation workspace of its own, so that the
        low-occupancy layers of one batch (stem, layer1, transitions, heads: HBM- and latency-bound) run beside the
        matrix-bound stages of the other - 14.5 -> 13.0-13.4 ms per forward at batch 32, 3.30 -> 2.13 ms at batch 1
        (`tools/two_stream_probe.py`).  The forwards of this loop run without the executor's parallel lanes (both at once
        are slower than either): a per-call flag, the process-wide option is not touched.  1 = every forward on the caller's stream.  ``exclusive(k)`` true: the forward of batch k
        runs alone - it starts when the forwards in flight are done and the next one starts behind it (bench.py times the
        kernels of such a step with per-op events: a kernel's duration beside another forward is not its own).

        ``out_hw``: as for ``__call__``, or a callable ``k -> (h, w) | [(h, w)] * N`` asked once per batch (before its
        forward), so that the decode sizes can change from batch to batch.

        Yields one ``[(people, scores)] * N`` list per batch, in order, two steps after the batch
        was submitted.  ``on_forward(k, x)`` may replace the plain forward (bench.py records op
        events); with ``flip_test`` it is called for the batch and for its mirror image, on the same stream,
        and T(k) is ``HeatmapParser.flip_topk`` of the pair.  With ``scale_factors`` every batch is a list of one tensor
        per scale; ``on_forward`` is called for every sub-batch (and its mirror image), all on the forward stream and
        workspace slot of step k; each sub-batch's maps are prepared on the decode stream as soon as its forwards are
        done (``HeatmapParser.ms_prep``) and T(k) is ``ms_topk``.  Keep the host thread pools small (``torch.set_num_threads``): a burst of idle-
        spinning OpenMP threads can exhaust a container's CPU quota and stall the launches.

        ``records``: a callable ``k -> (image_ids, xform | None)`` asked once per batch like ``out_hw`` (after the batch
        was taken from ``batches``, before its forward); needs ``match_on="device"``.  The generator then yields one
        (N, RECORD_FLOATS) record tensor per batch (class docstring) with the same two-step delay, safe to use on the
        stream that was current when the loop started: that stream is made to wait - on the device - for the event
        behind the record kernel.  The loop body then holds no host wait on decode work: every buffer of such a batch
        is device memory handed out again in stream order, or a pinned block reused only when its upload is done."""
        kind = self._kind(out_hw if callable(out_hw) else (lambda k: out_hw))
        return self._stream_loop(batches, kind, on_forward, decode_stream, in_flight, exclusive, records)

    def _stream_loop(self, batches, kind, on_forward, decode_stream, in_flight, exclusive, records):
        """the loop of ``stream()`` (its docstring), written once for every kind of batch: it knows streams, events,
        workspace slots and the two-step delay, and nothing of any protocol - that is ``kind`` (``_Kind``: ``begin``,
        ``tensors``, ``open``, ``forwards``, ``topk``), which gets ``on_decode_stream`` as its ``decode``.  The loop
        keeps each batch's state and checked ``records`` together until its grouping.  A generator."""
        import os
        mode = decode_stream or os.environ.get("RTPE_DECODE_STREAM", "side")
        if mode not in ("side", "same"):
            raise ValueError("decode_stream must be 'side' or 'same', not %r" % (mode,))
        main = torch.cuda.current_stream(self.device)
        n_fwd = int(in_flight if in_flight is not None else os.environ.get("RTPE_FORWARDS_IN_FLIGHT", "2"))
        if n_fwd < 1 or n_fwd > 4:
            raise ValueError("in_flight must be 1..4, not %r" % (n_fwd,))
        fwd_streams = None
        if n_fwd > 1:
            from .third_party.pose_higher_hrnet import (FWD_NO_LANES, forward_streams, set_forward_flags,
                                                        set_workspace_slot)
            # per device, not per pipeline: slot 1 + i of a model is always on stream i, whoever loops over it
            fwd_streams = forward_streams(self.device, n_fwd)
        side = None
        if mode == "side":
            side = self.__dict__.get("_decode_stream")
            if side is None:
                # normal priority (RTPE_DECODE_PRIORITY=-1: high).  A HIGH-priority decode stream beside the
                # forward's internal lane streams (option "lanes") more than halves the throughput - batch 1:
                # 123 img/s against 327, batch 32 with lanes on: 1,481 against 2,117 (profiles/r03_lanes_decode_stream.txt)
                # - and buys nothing without them (2,154 against 2,149)
                side = self._decode_stream = torch.cuda.Stream(
                    self.device, priority=int(os.environ.get("RTPE_DECODE_PRIORITY", "0")))
        after_alone = None    # the stream of an exclusive forward that the next forward has to wait for
        topk_done = None      # batch k-1: top-k enqueued
        refine_done = None    # batch k-2: refine enqueued
        P = self.parser

        def on_decode_stream(fn, *args, after=None, uses=()):
            if side is None:
                return fn(*args)
            with torch.cuda.stream(side):
                if after is not None:
                    side.wait_event(after)
                for t in uses:                  # allocated on the main stream, read on the side stream
                    t.record_stream(side)
                return fn(*args)

        # ``on_forward`` must return FRESH output tensors for every batch (the plain forward does): the decode of
        # batch k runs on the side stream while F(k+1) runs on the main one, and nothing makes F(k+1) wait for it.
        def match(st, rec):
            on_decode_stream(P.lowres_match, st, True, True, rec)

        def finish(st):
            out = P.lowres_finish(st)
            if records is not None and side is not None:
                main.wait_event(st["ev2"])          # a wait on the device: the host goes on
                out.record_stream(main)             # allocated on the decode stream, used on the caller's
            return out

        try:
            with torch.no_grad():
                for k, x in enumerate(batches):
                    x, hw = kind.begin(k, x)
                    rec_k = None
                    if records is not None:
                        ids_k, xf_k = records(k)
                        rec_k = self._records(kind.tensors(x)[0], ids_k, xf_k)
                    state = kind.open(x, hw, on_decode_stream)
                    fs = main
                    if fwd_streams is not None:
                        # forward k on stream k % n with workspace slot 1 + k % n; the input was produced on `main`
                        fs = fwd_streams[k % n_fwd]
                        fs.wait_stream(main)
                        alone = exclusive is not None and bool(exclusive(k))
                        if alone or after_alone is not None:
                            for other in fwd_streams[:n_fwd]:
                                if other is not fs:
                                    fs.wait_stream(other)
                        after_alone = fs if alone else None
                        for t in kind.tensors(x):
                            t.record_stream(fs)
                        # lanes off for THIS call only (a per-call flag of the ABI: nothing process-wide is touched,
                        # and nothing stays changed while the generator is suspended or if it is abandoned)
                        prev_slot = set_workspace_slot(1 + k % n_fwd)
                        prev_flags = set_forward_flags(0 if os.environ.get("RTPE_STREAM_LANES", "0") == "1" else FWD_NO_LANES)
                        try:
                            with torch.cuda.stream(fs):
                                outs = kind.forwards(k, x, on_forward, state, on_decode_stream)
                        finally:
                            set_forward_flags(prev_flags)
                            set_workspace_slot(prev_slot)
                    else:
                        outs = kind.forwards(k, x, on_forward, state, on_decode_stream)
                    f_done = None
                    if side is not None or fs is not main:
                        f_done = torch.cuda.Event()
                        f_done.record(fs)
                        if side is None:
                            main.wait_event(f_done)          # the decode runs on the caller's stream
                            for t in outs:
                                t.record_stream(main)
                    if topk_done is not None:
                        match(*topk_done)                               # host matching overlaps F(k) on the GPU
                    st = on_decode_stream(kind.topk, outs, hw, state, after=f_done, uses=outs)
                    if refine_done is not None:
                        yield finish(refine_done[0])
                    refine_done, topk_done = topk_done, (st, rec_k)
                if topk_done is not None:
                    match(*topk_done)
                if refine_done is not None:
                    yield finish(refine_done[0])
                if topk_done is not None:
                    yield finish(topk_done[0])
        finally:
            # also when the consumer stops early or an exception propagates: whoever continues on the main stream
            # sees the decode as done
            if side is not None:
                main.wait_stream(side)
            if fwd_streams is not None:
                for fs in fwd_streams[:n_fwd]:
                    main.wait_stream(fs)

    def gather(self, image_ids, results, equal_counts=False, force_collective=False):
        """all-gather of the decoded keypoints over the process group (RCCL).  ``equal_counts``:
        every rank contributes the same number of images (no count exchange, no host sync).
        ``force_collective``: issue the collective also in a process group of ONE rank (a world of one is
        otherwise answered locally; the switch lets a single GPU exercise the RCCL calls).  ``results`` may be the
        record tensor of ``__call__(..., image_ids=...)`` / ``stream(records=...)`` (``image_ids`` is then None): it is
        gathered where it lies."""
        if torch.is_tensor(results):            # device-resident records: they carry their ids, nothing to pack
            if image_ids is not None:
                raise ValueError("TeacherPipeline.gather: a record tensor carries its image ids; pass image_ids=None")
            if results.dim() != 2 or results.shape[1] != RECORD_FLOATS or results.dtype != torch.float32:
                raise ValueError("TeacherPipeline.gather: a record tensor is (n, %d) float32, not %s %s"
                                 % (RECORD_FLOATS, tuple(results.shape), results.dtype))
            rec = results
        else:
            rec = pack_records(image_ids, results, self.device)
        if not _collectives_on(force_collective):
            return rec
        return all_gather_records(rec, equal_counts)


class StudentPipeline(TeacherPipeline):
    """``TeacherPipeline`` for the dual-head students (rtpe/students.py ``AttentionStudent``, ``AttentionStudentSteps``;
    any module whose forward returns ``(att, det)`` with det (N, J + 1, h, w): J heat maps, then ONE tag map shared by
    all joints): batched forward on the HIP executor, then EVERY image of the batch decoded straight from ``det`` with
    ``HeatmapParser.parse_lowres_shared`` - no channel slice is copied and the tag map is never expanded.  Per image
    the result is bit-identical to what ``eval_student`` computes for image 0 of a batch,
    ``parse_lowres(det[:, :J].contiguous(), det[:, J:].expand(-1, J, -1, -1).contiguous(), out_hw)``.

    A batch is a tensor ``x`` (N,3,H,W) or a pair ``(x, alt)``, forwarded as ``model(x, alt=alt)`` (``alt``: the image
    in the alternative colour space; ``AttentionStudentSteps`` refuses to run without it).  ``stream()`` is
    ``TeacherPipeline.stream`` - the same loop, order, decode stream, forward streams / workspace slots, ``out_hw``
    callable and two-step delay; ``on_forward(k, batch)`` gets the batch as it was given and returns ``(att, det)``.
    One decode size per batch.  ``match_on`` as for ``TeacherPipeline``; ``gather`` is inherited.

    Images of different sizes: ``call_mixed(images)`` runs ONE forward over all of them (``AttentionStudent.forward_mixed``)
    and ONE decode, every image at its own size, straight from the output canvas (``HeatmapParser.parse_lowres_mixed``);
    ``stream_mixed(batches)`` is the pipelined loop over such batches and ``mixed_batches`` cuts a list of images into them.
    A model with a second input (``AttentionStudentSteps.forward_mixed``) gets it as ``call_mixed(images, alt=alts)``, as
    ``(images, alts)`` batches of ``stream_mixed`` and through ``mixed_batches(images, batch_size, alts=alts)``.
    ``stream()`` and ``__call__`` take one size per batch and refuse a mixed batch.

    The class supplies its kinds of batch - ``_StudentPlain`` through ``_kind``, ``_StudentMixed`` in ``stream_mixed``
    and ``call_mixed`` - and inherits the loop and the synchronous runner.

    There is no flip, multi-scale or AGS test protocol for the students: asking for one is a ValueError."""

    def __init__(self, model, parser=None, device=None, match_on=None, flip_test=False, scale_factors=None, ags=False,
                 project2image=True):
        if flip_test or scale_factors is not None or ags or not project2image:      # (before any GPU work)
            raise ValueError("StudentPipeline: flip_test, scale_factors, ags and project2image=False are test "
                             "protocols of the teacher; the students have the plain protocol only")
        super().__init__(model, parser, device, match_on=match_on)

    def _decode_hw(self, out_hw, images):
        # (the first thing ``__call__`` and every step of ``stream()`` do with a batch, before any GPU work)
        if self._is_mixed(images):
            raise ValueError("StudentPipeline: a mixed-size batch (a list of (3, h, w) images, a (canvas, sizes) pair) is "
                             "neither streamed nor decoded at one size; use call_mixed")
        hw = super()._decode_hw(out_hw, images)
        if hw is not None and len(hw) and hasattr(hw[0], "__len__"):
            raise ValueError("StudentPipeline: one decode size (h, w) per batch; per-image sizes are for the teacher's "
                             "plain protocol only")
        return hw

    @staticmethod
    def _att_det(out):
        """what a student's forward returned, checked: ``(att, det)`` with det (N, J + 1, h, w)"""
        if not isinstance(out, (list, tuple)) or len(out) != 2 or not torch.is_tensor(out[1]) or out[1].dim() != 4 or \
                out[1].shape[1] < 2:
            raise TypeError("StudentPipeline: the model must return (att, det) with det (N, J + 1, h, w)")
        return out[0], out[1]

    def _kind(self, out_hw_of):
        return _StudentPlain(self, out_hw_of)

    @staticmethod
    def _is_mixed(batch):
        """a list of (3, h, w) images, a (canvas, sizes) pair, an (images, alts) pair of two lists or a (canvas, sizes,
        alt_canvas) triple - what ``call_mixed`` / ``forward_mixed`` take"""
        if not isinstance(batch, (list, tuple)) or not batch:
            return False
        if torch.is_tensor(batch[0]) and batch[0].dim() == 3:
            return True
        if len(batch) == 3:
            return torch.is_tensor(batch[0]) and not torch.is_tensor(batch[1]) and batch[1] is not None
        return len(batch) == 2 and not torch.is_tensor(batch[1]) and batch[1] is not None

    def _mixed_model(self, who):
        """the one check of the model before a mixed batch is packed or launched: it has ``forward_mixed``, and not only to
        refuse it - a model that does (``AttentionStudentStepsHalf``) says so through ``refuse_mixed()``, raised here"""
        if not hasattr(self.model, "forward_mixed"):
            raise ValueError("%s: the model has no forward_mixed" % who)
        refuse = getattr(self.model, "refuse_mixed", None)
        if callable(refuse):
            refuse()

    @staticmethod
    def _mixed_batch(canvas, sizes, alt):
        """a mixed batch as ``forward_mixed`` and ``on_forward`` take it: ``(canvas, sizes[, alt_canvas])``"""
        return (canvas, sizes) if alt is None else (canvas, sizes, alt)

    def _mixed_takes_alt(self):
        """the model's ``forward_mixed`` has the second input ``alt`` (``AttentionStudentSteps``) and does not run without it"""
        import inspect
        try:
            return "alt" in inspect.signature(self.model.forward_mixed).parameters
        except (TypeError, ValueError):
            return False

    def _mixed_alt_given(self, given, who):
        """a model that needs the second input and gets none, or gets one and has no use for it: ValueError;
        otherwise ``given``"""
        if not given:
            if self._mixed_takes_alt():
                raise ValueError("%s: the model needs the second input of every image (alt: a list of (3, h_n, w_n) tensors "
                                 "of the images' sizes)" % who)
            return False
        if not self._mixed_takes_alt():
            raise ValueError("%s: the model's forward_mixed takes no second input (alt)" % who)
        return True

    def _mixed_alt(self, alts, sizes, canvas_hw, who):
        """the ``alt`` images of a mixed batch, checked against the images' sizes on the host and packed into a canvas of
        the first one's size; None stays None.  A model that needs them and gets none, or gets them and has no use for
        them, is refused here, before the forward."""
        from .students import pack_mixed
        if not self._mixed_alt_given(alts is not None, who):
            return None
        alts = list(alts)
        if len(alts) != len(sizes):
            raise ValueError("%s: %d alt images for %d images" % (who, len(alts), len(sizes)))
        for n, (a, hw) in enumerate(zip(alts, sizes)):
            if not torch.is_tensor(a) or a.dim() != 3 or a.shape[0] != 3 or tuple(a.shape[1:]) != tuple(hw):
                raise ValueError("%s: alt image %d must be a (3, %d, %d) tensor like its image, got %s"
                                 % (who, n, hw[0], hw[1], tuple(a.shape) if torch.is_tensor(a) else type(a).__name__))
        return pack_mixed(alts, canvas_hw=canvas_hw)[0]

    def _mixed_begin(self, batch):
        """a mixed batch as ``forward_mixed`` takes it, checked before the forward: a list of (3, h_n, w_n) images or an
        ``(images, alts)`` pair of two such lists is packed (``pack_mixed``, on the current stream), a ``(canvas, sizes)``
        pair or a ``(canvas, sizes, alt_canvas)`` triple checked -> ``((canvas, sizes[, alt_canvas]), sizes)``"""
        from .students import pack_mixed
        from .third_party.pose_higher_hrnet import check_mixed_sizes
        who = "StudentPipeline"
        self._mixed_model(who)
        if not self._is_mixed(batch):
            raise ValueError("StudentPipeline: a mixed-size batch is a list of (3, h, w) images or a (canvas, sizes) pair")
        one_list = torch.is_tensor(batch[0]) and batch[0].dim() == 3
        if one_list or (len(batch) == 2 and isinstance(batch[0], (list, tuple))):        # images, or (images, alts)
            images, alts = (batch, None) if one_list else batch
            canvas, sizes = pack_mixed(images)
            alt = self._mixed_alt(alts, sizes, tuple(canvas.shape[2:]), who)
        else:
            canvas, sizes, alt = batch[0], batch[1], batch[2] if len(batch) == 3 else None
            if not torch.is_tensor(canvas) or canvas.dim() != 4 or canvas.shape[1] != 3:
                raise ValueError("StudentPipeline: the canvas of a mixed batch is (N,3,Hc,Wc)")
            sizes = check_mixed_sizes(sizes, canvas.shape[0], canvas.shape[2], canvas.shape[3])
            if self._mixed_alt_given(alt is not None, who) and (
                    not torch.is_tensor(alt) or tuple(alt.shape) != tuple(canvas.shape) or alt.device != canvas.device):
                raise ValueError("StudentPipeline: the alt canvas of a mixed batch is a tensor like the first canvas, %s on %s"
                                 % (tuple(canvas.shape), canvas.device))
        return self._mixed_batch(canvas, sizes, alt), sizes

    def _mixed_forwards(self, k, batch, on_forward):
        att, det = self._att_det(on_forward(k, batch) if on_forward is not None else self.model.forward_mixed(*batch))
        if det.shape[0] != batch[0].shape[0]:
            raise TypeError("StudentPipeline: det %s is not the canvas of the %d images of the batch"
                            % (tuple(det.shape), batch[0].shape[0]))
        return att, det

    @torch.no_grad()
    def call_mixed(self, images, image_ids=None, decode="batch", alt=None):
        """images: a list of (3, h_n, w_n) tensors on the GPU, any sizes >= 32 [, ``alt``: the list of the same images in
        the alternative colour space, same sizes, for a model with a second input] -> per image what ``self(x_n[None])``
        (``self(x_n[None], alt=alt_n[None])``) returns for it: ``pack_mixed``, ONE ``forward_mixed``, then ONE decode of
        the whole batch straight from the ``det``
        canvas, every image at its own (h_n, w_n) from its own region (``HeatmapParser.parse_lowres_mixed``: nothing is
        copied).  ``decode="per_image"``: every image decoded on its own with ``parse_lowres_shared`` from a contiguous copy
        of its region - N region copies, N sets of launches and 2N host waits in series; the same bits, kept for A/B
        measurements and as a fallback.  With ``image_ids`` (N ints; ``match_on="device"``): one (1, RECORD_FLOATS) record
        tensor per image (``"batch"``: views of the one record tensor of the batch)."""
        from .students import pack_mixed
        who = "StudentPipeline.call_mixed"
        self._mixed_call_checks(decode, who)
        canvas, sizes = pack_mixed(images)
        return self._mixed_call(who, canvas, sizes, lambda: self._mixed_alt(alt, sizes, tuple(canvas.shape[2:]), who),
                                image_ids, decode)

    def _mixed_call_checks(self, decode, who):
        """what ``call_mixed`` and ``call_frames`` refuse before anything is packed"""
        if decode not in ("batch", "per_image"):
            raise ValueError("%s: decode must be 'batch' or 'per_image', not %r" % (who, decode))
        self._mixed_model(who)

    def _mixed_call(self, who, canvas, sizes, alt_canvas, image_ids, decode):
        """``call_mixed`` from its first canvas on: the count of the image ids, the second canvas (``alt_canvas()``: asked
        for behind that check, where ``call_mixed`` has always packed it), ONE ``forward_mixed``, then the decode"""
        from .students import unpack_mixed
        if image_ids is not None and len(image_ids) != len(sizes):
            raise ValueError("%s: %d image ids for %d images" % (who, len(image_ids), len(sizes)))
        batch = self._mixed_batch(canvas, sizes, alt_canvas())
        if decode == "batch":
            res = self._run(_StudentMixed(self, packed=True), batch, image_ids)
            return res if image_ids is None else [res[n:n + 1] for n in range(len(sizes))]
        records = [None if image_ids is None else self.parser.check_records(1, ([image_ids[n]], None))
                   for n in range(len(sizes))]
        att, det = self._mixed_forwards(0, batch, None)
        out = []
        for n, (_, d) in enumerate(unpack_mixed(att, det, sizes)):
            d = d.unsqueeze(0).float().contiguous()
            J = d.shape[1] - 1
            res = self.parser.parse_lowres_shared(d[:, :J], d[:, J:], sizes[n], records=records[n])
            out.append(res if records[n] is not None else res[0])
        return out

    def stream_mixed(self, batches, on_forward=None, decode_stream=None, in_flight=None, exclusive=None, records=None):
        """``stream()`` over mixed-size batches: the same software-pipelined loop F(k) R(k-1) T(k) - decode stream,
        forward streams and workspace slots, ``exclusive``, early stop, two-step delay of the results - with
        F = ``forward_mixed`` and T = ``HeatmapParser.lowres_topk_mixed`` on the ``det`` canvas.  Every batch is a list of
        (3, h_n, w_n) images (packed on the caller's stream) or a ``(canvas, sizes)`` pair (``pack_mixed``); for a model
        with a second input an ``(images, alts)`` pair of two lists or a ``(canvas, sizes, alt_canvas)`` triple.  Every image
        is decoded at its own size.  ``on_forward(k, (canvas, sizes[, alt_canvas]))`` may replace the forward and returns
        ``(att, det)``.
        Yields per batch what ``call_mixed`` returns for it, or with ``records`` (``k -> (image_ids, None)``; needs
        ``match_on="device"``) the (N, RECORD_FLOATS) record tensor of the batch."""
        return self._stream_loop(batches, _StudentMixed(self), on_forward, decode_stream, in_flight, exclusive, records)

    @torch.no_grad()
    def call_frames(self, frames, alt_colorspace=None, image_ids=None, decode="batch"):
        """``call_mixed`` from uint8 frames: ``frames`` a sequence of (h_n, w_n, 3) uint8 ndarrays, CPU tensors or device
        tensors of any sizes >= 32 (or one (N, H, W, 3) array) -> per image what ``call_mixed`` returns for
        ``Normalize(to_tensor(frame))`` [and, for a model with a second input, ``alt_colorspace`` "LAB" / "HSV": the
        image in that colour space].  ``students.pack_frames`` - one upload and one launch write both canvases - then
        exactly what ``call_mixed`` does from its canvases on; ``image_ids`` and ``decode`` as there."""
        from .students import pack_frames
        who = "StudentPipeline.call_frames"
        self._mixed_call_checks(decode, who)
        self._mixed_alt_given(alt_colorspace is not None, who)
        canvas, sizes, alt = pack_frames(frames, alt_colorspace, device=self.device)
        return self._mixed_call(who, canvas, sizes, lambda: alt, image_ids, decode)

    def stream_frames(self, batches, alt_colorspace=None, **stream_mixed_kwargs):
        """``stream_mixed`` over batches of uint8 frames (each what ``call_frames`` takes; ``frame_batches`` cuts them):
        every batch goes through ``students.pack_frames`` on the caller's stream when the loop reaches it and enters
        ``stream_mixed`` as ``(canvas, sizes[, alt_canvas])``.  ``alt_colorspace`` as ``call_frames``; every other
        argument is ``stream_mixed``'s."""
        from .students import pack_frames
        who = "StudentPipeline.stream_frames"
        self._mixed_model(who)
        self._mixed_alt_given(alt_colorspace is not None, who)

        def packed():
            for frames in batches:
                yield self._mixed_batch(*pack_frames(frames, alt_colorspace, device=self.device))
        return self.stream_mixed(packed(), **stream_mixed_kwargs)

    @staticmethod
    def mixed_batches(images, batch_size=32, alts=None):
        """cut a list of images of different sizes into batches for ``call_mixed`` / ``stream_mixed``: the images
        sorted by area (so that a canvas wastes little on its smaller images; ties keep the caller's order), then runs
        of ``batch_size``.  ``images``: (3, h, w) tensors, or anything with such a ``.shape``.  Returns
        ``(batches, restore)``: ``batches[b]`` the list of images of batch b, and ``restore(results)`` - ``results[b]`` the
        per-image list that batch b gave - the results of all images in the caller's order.  With ``alts`` (one per image,
        for a model with a second input) they are cut in the same order and ``batches[b]`` is the pair ``(images, alts)``
        of batch b, as ``stream_mixed`` takes it.  Pure host function."""
        return StudentPipeline._area_batches(images, batch_size, alts, lambda s: int(s[-2]) * int(s[-1]),
                                             "StudentPipeline.mixed_batches")

    @staticmethod
    def frame_batches(frames, batch_size=32):
        """``mixed_batches`` for (h, w, 3) frames, what ``call_frames`` / ``stream_frames`` take: sorted by ``h * w``
        (``mixed_batches`` would read ``w * 3`` from such a shape), ties keep the caller's order, then runs of
        ``batch_size``.  ``frames``: anything with an (h, w, 3) ``.shape``.  Returns ``(batches, restore)`` as
        ``mixed_batches`` does.  Pure host function."""
        return StudentPipeline._area_batches(frames, batch_size, None, lambda s: int(s[0]) * int(s[1]),
                                             "StudentPipeline.frame_batches")

    @staticmethod
    def _area_batches(images, batch_size, alts, area, who):
        images = list(images)
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("%s: batch_size must be at least 1, not %d" % (who, batch_size))
        if alts is not None:
            alts = list(alts)
            if len(alts) != len(images):
                raise ValueError("%s: %d alts for %d images" % (who, len(alts), len(images)))
        order = sorted(range(len(images)), key=lambda i: area(images[i].shape))
        cuts = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]

        def restore(results):
            results = list(results)
            if len(results) != len(cuts) or any(len(r) != len(c) for r, c in zip(results, cuts)):
                raise ValueError("%s: the results %s do not go with batches of %s images"
                                 % (who, [len(r) for r in results], [len(c) for c in cuts]))
            out = [None] * len(images)
            for r, c in zip(results, cuts):
                for i, v in zip(c, r):
                    out[i] = v
            return out
        if alts is not None:
            return [([images[i] for i in c], [alts[i] for i in c]) for c in cuts], restore
        return [[images[i] for i in c] for c in cuts], restore

    def __call__(self, images, out_hw=None, alt=None, image_ids=None, xform=None):
        """images (N,3,H,W) on the GPU [, alt (N,3,H,W)] -> list of (people, scores) for all N images; out_hw = the
        decode resolution (h, w), default (H, W); with ``image_ids`` [and ``xform``] the record tensor, as
        ``TeacherPipeline.__call__``"""
        # (a mixed-size batch goes alone: it is refused as one, with or without ``alt``)
        batch = images if alt is None or self._is_mixed(images) else (images, alt)
        return self._run(self._kind(lambda k: out_hw), batch, image_ids, xform)


def _collectives_on(force_collective=False):
    """a process group is up and has more than one rank - or one rank and the caller insists"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or bool(force_collective)


def _collective_tensor(t):
    """RCCL moves device memory; gloo (CPU rehearsals, or several ranks sharing one GPU) wants host memory"""
    import torch.distributed as dist
    if t.is_cuda and dist.get_backend() == "gloo":
        return t.cpu(), t.device
    return t, None


def all_gather_records(rec, equal_counts=False):
    """records of all ranks, in rank order.  Variable count per rank: pad to the max, gather,
    strip the padding (one count exchange that the host has to read); with ``equal_counts`` a
    single collective and nothing for the host to wait for."""
    import torch.distributed as dist
    world = dist.get_world_size()
    rec, home = _collective_tensor(rec)
    if home is not None:
        return all_gather_records(rec, equal_counts).to(home)
    if equal_counts:
        out = torch.empty((world * rec.shape[0], rec.shape[1]), dtype=rec.dtype, device=rec.device)
        dist.all_gather_into_tensor(out, rec.contiguous())
        return out
    n = torch.tensor([rec.shape[0]], dtype=torch.int64, device=rec.device)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n)
    m = int(max(int(c.item()) for c in counts))
    pad = torch.zeros((m, rec.shape[1]), dtype=rec.dtype, device=rec.device)
    pad[:rec.shape[0]] = rec
    out = torch.empty((world * m, rec.shape[1]), dtype=rec.dtype, device=rec.device)
    dist.all_gather_into_tensor(out, pad)
    keep = [out[r * m:r * m + int(counts[r].item())] for r in range(world)]
    return torch.cat(keep)


# --------------------------------------------------------------------------- #
# teacher-prediction files (teacher_inference.py:67-90 writes them, dataloaders.py:140-165 reads them)
# --------------------------------------------------------------------------- #
HEATMAPS_ORDER = ["nose", "leye", "reye", "lear", "rear", "lshould", "rshould", "lelbow", "relbow", "lwrist",
                  "rwrist", "lhip", "rhip", "lknee", "rknee", "lankle", "rankle"]   # teacher_inference.py:38-40


def teacher_prediction_path(out_dir, img_path):
    """teacher_inference.py:68-69; numpy appends ``.npz``, the reader asks for
    ``<img_id>.jpg_w48_predictions.npz`` (dataloaders.py:149-150)"""
    import os
    return os.path.join(out_dir, os.path.basename(img_path)) + "_w48_predictions"


def save_teacher_predictions(out_path, preds, refined):
    """teacher_inference.py:83-90: ``preds`` (34,h,w) and ``refined`` (17,2h,2w) of ONE image (tensors or
    arrays, a leading batch axis of 1 is squeezed) -> compressed npz with the reference's four keys"""
    preds = np.asarray(preds.detach().cpu() if torch.is_tensor(preds) else preds, np.float32).squeeze()
    refined = np.asarray(refined.detach().cpu() if torch.is_tensor(refined) else refined, np.float32).squeeze()
    if preds.ndim != 3 or preds.shape[0] != 2 * NUM_HEATMAPS or refined.ndim != 3 or refined.shape[0] != NUM_HEATMAPS:
        raise ValueError("save_teacher_predictions: expected (34,h,w) and (17,H,W), got %s and %s"
                         % (preds.shape, refined.shape))
    np.savez_compressed(out_path, pred_heatmaps=preds[:NUM_HEATMAPS], embeddings=preds[NUM_HEATMAPS:],
                        heatmaps_refined=refined, heatmaps_order=HEATMAPS_ORDER)


def load_teacher_predictions(path, out_hw=None, device=None):
    """dataloaders.py:140-165 ``_get_teacher_data``: -> ``(t_hms, t_ae)`` float32 tensors
    ``heatmaps_refined`` (17,H,W) and ``embeddings`` (17,h,w); with ``out_hw`` both are upsampled with
    ``F.interpolate(mode="bilinear", align_corners=True)`` semantics on the GPU (``device`` required)."""
    npz = np.load(path if str(path).endswith(".npz") else str(path) + ".npz")
    t_hms = torch.from_numpy(np.ascontiguousarray(npz["heatmaps_refined"], np.float32))
    t_ae = torch.from_numpy(np.ascontiguousarray(npz["embeddings"], np.float32))
    if device is not None:
        t_hms, t_ae = t_hms.to(device), t_ae.to(device)
    if out_hw is not None:
        from .third_party.group import upsample_bilinear
        t_hms = upsample_bilinear(t_hms.unsqueeze(0), out_hw)[0]
        t_ae = upsample_bilinear(t_ae.unsqueeze(0), out_hw)[0]
    return t_hms, t_ae


def export_teacher_predictions(model, items, out_dir, workers=4):
    """teacher_inference.py:67-90 as a loop: ``items`` yields ``(img_path, t)`` with ``t`` (1,3,H,W) on
    the GPU (see ``rtpe.third_party.transforms.warp_normalize``).  The forward of the next image is
    enqueued while a small thread pool compresses and writes the previous ones (the ~3 MB of
    deflate per image is the cost of this path).  Returns the list of files written."""
    from concurrent.futures import ThreadPoolExecutor
    written, futures = [], []
    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool, torch.no_grad():
        for img_path, t in items:
            preds, refined = model(t)
            out_path = teacher_prediction_path(out_dir, img_path)
            p_host = torch.empty(preds.shape, dtype=torch.float32, pin_memory=True)
            r_host = torch.empty(refined.shape, dtype=torch.float32, pin_memory=True)
            p_host.copy_(preds, non_blocking=True)
            r_host.copy_(refined, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()

            def job(ev=ev, p=p_host, r=r_host, path=out_path):
                ev.synchronize()
                save_teacher_predictions(path, p.numpy(), r.numpy())
                return path + ".npz"
            futures.append(pool.submit(job))
        for f in futures:
            written.append(f.result())
    return written


def shard_indices(n_items, rank, world):
    """contiguous blocks, sizes differing by at most one (100 images over 8 ranks
    -> 13,13,13,13,12,12,12,12)"""
    base, extra = divmod(n_items, world)
    start = rank * base + min(rank, extra)
    return list(range(start, start + base + (1 if rank < extra else 0)))


def image_id_of(name):
    """COCO image id of a file name such as ``000000576052.jpg`` (the entries of
    assets/coco_minival2017_100.txt of the reference); the id is what travels in the keypoint records"""
    import os
    stem = os.path.splitext(os.path.basename(str(name).strip()))[0]
    return int(stem)


def run_sharded_list(names, infer, batch_size, device, force_collective=False):
    """configs[3]: one image list, one process per GPU.  ``names`` is the WHOLE list, identical on every rank;
    this rank takes its contiguous block (``shard_indices``: 100 names over 8 ranks -> 13,13,13,13,12,12,12,12),
    runs it in batches of ``batch_size`` (the last batch of a shard is short, the shards are uneven) through
    ``infer(list_of_names) -> [(people, scores)] per name``, and the decoded keypoints of ALL ranks are
    all-gathered as fixed-size records, with a count exchange because the shards differ in length.  No other
    collective touches the data path.  Returns ``{image_id: (kpts (P,17,4), scores (P))}`` for the whole list
    on every rank, after checking that every image of the list came back exactly once.  ``force_collective``: run
    the count exchange and the gather also when the process group has a single rank."""
    import torch.distributed as dist
    on = _collectives_on(force_collective)
    rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
    mine = shard_indices(len(names), rank, world)
    ids = [image_id_of(names[i]) for i in range(len(names))]
    if len(set(ids)) != len(ids):
        raise ValueError("run_sharded_list: duplicate image ids in the list")
    recs = []
    for o in range(0, len(mine), batch_size):
        part = mine[o:o + batch_size]
        results = infer([names[i] for i in part])
        if len(results) != len(part):
            raise RuntimeError("run_sharded_list: infer returned %d results for %d images" % (len(results), len(part)))
        recs.append(pack_records([ids[i] for i in part], results, device))
    rec = torch.cat(recs) if recs else torch.zeros((0, RECORD_FLOATS), dtype=torch.float32, device=device)
    allrec = all_gather_records(rec) if on else rec
    out = unpack_records(allrec)
    got = [int(r) for r in allrec[:, 0].cpu().tolist()]
    if sorted(got) != sorted(ids):
        missing = sorted(set(ids) - set(got))
        dup = sorted({g for g in got if got.count(g) > 1})
        raise RuntimeError("run_sharded_list: gathered %d records for %d images (missing %s, duplicated %s)"
                           % (len(got), len(ids), missing[:5], dup[:5]))
    return out


def broadcast_state_dict(sd, src=0, device=None, force_collective=False):
    """rank ``src`` holds the checkpoint; every rank gets the tensors over
    RCCL as ONE packed buffer per dtype.  ``force_collective``: broadcast also in a
    process group of one rank."""
    import torch.distributed as dist
    if not _collectives_on(force_collective):
        return sd
    keys = sorted(sd.keys())
    out = {}
    for dt in (torch.float32, torch.float16, torch.int64):
        ks = [k for k in keys if sd[k].dtype == dt]
        if not ks:
            continue
        flat = torch.cat([sd[k].reshape(-1) for k in ks]).to(device)
        flat, home = _collective_tensor(flat)
        dist.broadcast(flat, src)
        o = 0
        for k in ks:
            n = sd[k].numel()
            out[k] = flat[o:o + n].reshape(sd[k].shape).cpu()
            o += n
    return out
