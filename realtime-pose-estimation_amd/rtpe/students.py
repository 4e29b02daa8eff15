"""The dual-head student of config 5 on MI355X.

Drop-in for the parts of the reference's ``rtpe/students.py`` that
``BASELINE.json`` configs[4] exercises: ``SELayer`` (:118-142),
``ContextAwareModule`` (:145-201), ``StemHRNet`` (:206-283),
``get_pretrained_stem`` (:286-298), ``init_weights`` (:20-32) and
``AttentionStudent`` (:595-771) - same constructor signatures, same attribute
names (hence the same state-dict keys: the bundled
``assets/pretrained_segm_4MB/*.statedict`` load through ``load_state_dicts``),
same ``forward(x, out_hw=None, return_intermediate=False) -> (att, det)``.
The other student classes of that file are abandoned experiments (SURVEY.md
section 2) and are not built.

As for the teacher, the ``torch.nn`` leaves only hold parameters; ``forward``
compiles the tree into one program (fp16 stem under the half wrapper, then a
cast, then fp32 ops: dilated 3x3 convs on the exact-fp32 MFMA, SE gates, CAM
combine, average pooling, sigmoid; with ``AttentionStudent(body_half=True)`` no
cast and the fp16 forms of the same ops) and runs it on the HIP executor.  The quirks
of the reference forward are reproduced as they are (``AttentionStudentStepsHalf``: the Steps student with an fp16 body,
a class of its own): ``att = hi + 2*up(lo)``
(:739-742), ``det_hi`` used for both ``hi`` and ``mid`` and ``det_mid`` never
called (:759-760).
"""
import torch

from . import _native as nat
from .third_party.fp16_utils.fp16util import BN_convert_float, network_to_half, tofp16
from .third_party.pose_higher_hrnet import BN_MOMENTUM, Bottleneck, CompiledModule, ProgramBuilder, check_mixed_sizes
from .third_party.transforms import IMAGENET_MEAN, IMAGENET_STD


def _canvas_hw(sizes, canvas_hw=None):
    """(Hc, Wc) of the canvas of a batch of images of ``sizes``: the largest h_n and w_n, or ``canvas_hw`` as it is given
    (whether it holds the images is for the caller to check, in its own words)"""
    if canvas_hw is not None:
        return int(canvas_hw[0]), int(canvas_hw[1])
    return max(h for h, _ in sizes), max(w for _, w in sizes)


def pack_mixed(images, canvas_hw=None):
    """images of different sizes -> one canvas for ``AttentionStudent.forward_mixed``.

    ``images``: a list of (3, h_n, w_n) tensors on one device, h_n, w_n >= 32.  Returns ``(canvas, sizes)``: canvas
    (N, 3, Hc, Wc) float32 with image n at ``[n, :, :h_n, :w_n]`` and zeros elsewhere, ``sizes = [(h_n, w_n)]``.
    ``Hc, Wc`` are the largest h_n and w_n, or ``canvas_hw`` (not smaller than those)."""
    images = list(images)
    if not images:
        raise ValueError("pack_mixed: no images")
    for n, im in enumerate(images):
        if not torch.is_tensor(im) or im.dim() != 3 or im.shape[0] != 3:
            raise ValueError("pack_mixed: image %d must be a (3, h, w) tensor" % n)
        if im.device != images[0].device:
            raise ValueError("pack_mixed: images on different devices (%s and %s)" % (images[0].device, im.device))
    sizes = [(int(im.shape[1]), int(im.shape[2])) for im in images]
    (Hc, Wc), (Hm, Wm) = _canvas_hw(sizes, canvas_hw), _canvas_hw(sizes)
    if Hc < Hm or Wc < Wm:
        raise ValueError("pack_mixed: a %d x %d canvas does not hold images of up to %d x %d" % (Hc, Wc, Hm, Wm))
    sizes = check_mixed_sizes(sizes, len(images), Hc, Wc)
    canvas = torch.zeros((len(images), 3, Hc, Wc), dtype=torch.float32, device=images[0].device)
    for n, (im, (h, w)) in enumerate(zip(images, sizes)):
        canvas[n, :, :h, :w] = im
    return canvas, sizes


def _frame_kind(frame, n):
    """"device" / "host" for an (h, w, 3) uint8 tensor on a GPU / ndarray or CPU tensor; TypeError for anything else"""
    import numpy as np
    is_t = torch.is_tensor(frame)
    if not (is_t or isinstance(frame, np.ndarray)) or frame.dtype != (torch.uint8 if is_t else np.uint8) \
            or len(frame.shape) != 3 or frame.shape[2] != 3:
        raise TypeError("pack_frames: frame %d: expected an (h, w, 3) uint8 ndarray or tensor, got %s %s"
                        % (n, getattr(frame, "dtype", type(frame).__name__), tuple(getattr(frame, "shape", ()))))
    return "device" if is_t and frame.is_cuda else "host"


def pack_frames(frames, alt_colorspace=None, canvas_hw=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda",
                out=None):
    """uint8 frames of different sizes, as a camera or an image decoder delivers them -> the canvases of
    ``forward_mixed(canvas, sizes, alt=alt_canvas)``, in one upload and ONE kernel launch (``rtpe_frames_to_canvases``).

    ``frames``: a sequence of (h_n, w_n, 3) uint8 ndarrays, CPU tensors or tensors on the device, freely mixed, or one
    (N, H, W, 3) uint8 array / tensor (the same-size case); h_n, w_n >= 32.  Returns ``(canvas, sizes, alt_canvas)``:
    ``canvas`` (N, 3, Hc, Wc) float32 with ``Normalize(mean, std)(to_tensor(frame n))`` at ``[n, :, :h_n, :w_n]`` - the
    bits of ``(float32(f) / 255 - mean) / std`` in numpy float32 or torch on the CPU, two true divisions - and
    ``alt_canvas`` the same region in ``alt_colorspace`` ("LAB" / "HSV": the bits of ``dataloaders.rgb2lab`` /
    ``rgb2hsv`` of ``to_tensor(frame n)``), or None without one.  Every other element of both canvases is exactly 0.0,
    written by the same kernel: the canvases are ``torch.empty``.  ``Hc, Wc`` are the largest h_n and w_n, or
    ``canvas_hw`` (not smaller than those); ``sizes = [(h_n, w_n)]``.

    Host frames are copied behind the job table into one pinned staging slot (the ring of
    ``transforms.warp_normalize_batch``) and go up with one asynchronous copy; frames on the device are read where they
    lie (any row stride >= 3 * w; made contiguous only if the pixel stride is not 3).  Everything is queued on the
    current stream.  ``out=(canvas, alt_canvas)`` (``alt_canvas`` None without a colour space): caller-owned contiguous
    float32 tensors of the right shape on the device, written instead of fresh ones - for a loop that reuses its buffers.

    Frames of ONE size give a plain (N, 3, H, W) batch: ``pipe(canvas, alt=alt_canvas)`` and every student class,
    ``AttentionStudentStepsHalf`` included, take it as they take any tensor.

    Refused before any GPU work: no frames, a side below 32, a canvas too small, an ``out`` of the wrong shape, dtype or
    device (ValueError); a frame that is not (h, w, 3) uint8 (TypeError); an unknown colour space (NotImplementedError)."""
    import ctypes
    import numpy as np
    from .third_party.transforms import _staging_slot
    if (torch.is_tensor(frames) or isinstance(frames, np.ndarray)) and len(frames.shape) == 4:
        frames = [frames[n] for n in range(frames.shape[0])]
    elif torch.is_tensor(frames) or isinstance(frames, np.ndarray):
        raise TypeError("pack_frames: a sequence of (h, w, 3) uint8 frames or one (N, H, W, 3) array, not one %s array"
                        % (tuple(frames.shape),))
    frames = list(frames)
    if not frames:
        raise ValueError("pack_frames: no frames")
    if alt_colorspace not in nat.FRAMES_ALT_MODES:
        raise NotImplementedError("Unknown color space {}".format(alt_colorspace))
    mode = nat.FRAMES_ALT_MODES[alt_colorspace]
    kinds = [_frame_kind(f, n) for n, f in enumerate(frames)]
    N = len(frames)
    sizes = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
    Hc, Wc = _canvas_hw(sizes, canvas_hw)
    sizes = check_mixed_sizes(sizes, N, Hc, Wc)
    if len(mean) != 3 or len(std) != 3 or not all(float(s) > 0 for s in std):
        raise ValueError("pack_frames: mean and std are three numbers each, std positive")
    device = torch.device(device)
    if out is not None:
        if not isinstance(out, (list, tuple)) or len(out) != 2 or (out[1] is None) != (mode < 0):
            raise ValueError("pack_frames: out is (canvas, alt_canvas), alt_canvas None exactly when there is no "
                             "colour space")
        for name, t in (("canvas", out[0]), ("alt_canvas", out[1])):
            if t is None and name == "alt_canvas":
                continue
            if not torch.is_tensor(t) or tuple(t.shape) != (N, 3, Hc, Wc) or t.dtype != torch.float32 or \
                    not t.is_contiguous() or t.device.type != device.type or \
                    (device.index is not None and t.device.index != device.index) or t.device != out[0].device:
                raise ValueError("pack_frames: out: %s must be a contiguous float32 tensor %s on %s, got %s"
                                 % (name, (N, 3, Hc, Wc), device, "%s %s on %s" % (t.dtype, tuple(t.shape), t.device)
                                    if torch.is_tensor(t) else type(t).__name__))
        device = out[0].device
    if device.type != "cuda":
        raise RuntimeError("rtpe: pack_frames runs on the MI355X HIP path only and got device %s (there is "
                           "deliberately no CPU fallback in the product path)" % (device,))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    L = nat.lib()
    tb = ctypes.c_size_t()
    nat.check(L.rtpe_frames_table_bytes(N, ctypes.byref(tb)))
    # the staging buffer: [job table | host frame 0 | host frame 1 | ...], frames packed (row stride 3 * w)
    offsets, total = {}, (tb.value + 255) // 256 * 256
    for n, (h, w) in enumerate(sizes):
        if kinds[n] == "host":
            offsets[n] = total
            total += (h * w * 3 + 15) // 16 * 16
    with torch.cuda.device(device):
        slot = _staging_slot(device, total)
        host = slot["buf"]
        host_np = host.numpy()
        stage = torch.empty(total, dtype=torch.uint8, device=device)
        canvas, alt = out if out is not None else (
            torch.empty((N, 3, Hc, Wc), dtype=torch.float32, device=device),
            torch.empty((N, 3, Hc, Wc), dtype=torch.float32, device=device) if mode >= 0 else None)
        src_addr = (ctypes.c_uint64 * N)()
        src_hws = (ctypes.c_int32 * (3 * N))()
        keep = []           # device frames and their contiguous copies: alive until the launch is in the stream
        for n, (f, (h, w)) in enumerate(zip(frames, sizes)):
            if kinds[n] == "host":
                np.copyto(host_np[offsets[n]:offsets[n] + h * w * 3].reshape(h, w, 3),
                          f.numpy() if torch.is_tensor(f) else f)
                src_addr[n], stride = stage.data_ptr() + offsets[n], 3 * w
            else:
                if f.device != device:
                    raise RuntimeError("rtpe: pack_frames: frame %d is on %s, the canvases are on %s" % (n, f.device, device))
                if f.stride(2) != 1 or f.stride(1) != 3 or f.stride(0) < 3 * w:
                    f = f.contiguous()
                keep.append(f)
                src_addr[n], stride = f.data_ptr(), f.stride(0)
            src_hws[3 * n], src_hws[3 * n + 1], src_hws[3 * n + 2] = h, w, stride
        nat.check(L.rtpe_frames_table_fill(src_addr, src_hws, N, Hc, Wc, ctypes.c_void_p(host.data_ptr()), tb.value))
        # (all frames on the device: only the table goes up)
        stage.copy_(host[:total], non_blocking=True)
        if slot["event"] is None:
            slot["event"] = torch.cuda.Event()
        slot["event"].record(torch.cuda.current_stream(device))
        nat.check(L.rtpe_frames_to_canvases(
            ctypes.c_void_p(stage.data_ptr()), N, Hc, Wc, (ctypes.c_float * 3)(*[float(v) for v in mean]),
            (ctypes.c_float * 3)(*[float(v) for v in std]), mode, ctypes.c_void_p(canvas.data_ptr()),
            ctypes.c_void_p(alt.data_ptr()) if alt is not None else None, nat.stream_ptr(device)))
        del keep
    return canvas, sizes, alt


def unpack_mixed(att, det, sizes):
    """the output canvases of ``forward_mixed`` -> ``[(att_n, det_n)]``: per image the views
    ``[n, :, :ceil(h_n / 4), :ceil(w_n / 4)]`` (nothing is copied)"""
    sizes = check_mixed_sizes(sizes, att.shape[0], att.shape[2] * 4, att.shape[3] * 4)
    if det.shape[0] != att.shape[0] or det.shape[2:] != att.shape[2:]:
        raise ValueError("unpack_mixed: att %s and det %s are not one batch" % (tuple(att.shape), tuple(det.shape)))
    out = []
    for n, (h, w) in enumerate(sizes):
        eh, ew = nat.extent(h, 2), nat.extent(w, 2)
        out.append((att[n, :, :eh, :ew], det[n, :, :eh, :ew]))
    return out


def init_weights(module, init_fn=torch.nn.init.kaiming_normal_, bias_val=0.0):
    """reference :20-32"""
    if isinstance(module, (torch.nn.Linear, torch.nn.Conv2d)):
        init_fn(module.weight)
        if module.bias is not None:
            module.bias.data.fill_(bias_val)


class SELayer(torch.nn.Module):
    """squeeze-excitation gate (reference :118-142): returns the (N,C,1,1) gate only"""

    def __init__(self, in_chans, hidden_chans=None, bn_momentum=0.1):
        super().__init__()
        hidden_chans = in_chans // 4 if hidden_chans is None else hidden_chans
        self.avg_pool = torch.nn.AdaptiveAvgPool2d(1)
        self.fc = torch.nn.Sequential(torch.nn.Linear(in_chans, hidden_chans, bias=True),
                                      torch.nn.ReLU(inplace=True),
                                      torch.nn.Linear(hidden_chans, in_chans, bias=True),
                                      torch.nn.Sigmoid())

    def emit(self, b, x, w1=None):
        return b.se(x, self.fc[0], self.fc[2], w1=w1)

    def forward(self, x):
        raise RuntimeError("rtpe: SELayer runs only inside a compiled student program")


def _cbr(cin, cout, k, dilation=1, bn_momentum=0.1):
    return torch.nn.Sequential(
        torch.nn.Conv2d(cin, cout, kernel_size=k, stride=1, dilation=dilation,
                        padding=dilation * (k // 2), bias=False),
        torch.nn.BatchNorm2d(cout, momentum=bn_momentum), torch.nn.ReLU(inplace=True))


class ContextAwareModule(torch.nn.Module):
    """CAM (reference :145-201): relu(residual(x) + hdc_top(cat(hdc_d(x))) * se(x))"""

    def __init__(self, in_chans, se_chans=None, hdc_dilations=[1, 2, 3, 4], hdc_chans=None, bn_momentum=0.1):
        super().__init__()
        self.residual = _cbr(in_chans, in_chans, 1, bn_momentum=bn_momentum)
        self.se = SELayer(in_chans, se_chans, bn_momentum)
        hdc_chans = in_chans // 4 if hdc_chans is None else hdc_chans
        self.hdcs = torch.nn.ModuleList([_cbr(in_chans, hdc_chans, 3, d, bn_momentum) for d in hdc_dilations])
        self.hdc_top = _cbr(hdc_chans * len(hdc_dilations), in_chans, 1, bn_momentum=bn_momentum)
        self.final_relu = torch.nn.ReLU(inplace=True)

    def emit(self, b, x, col_map=None):
        """``col_map``: physical channel of x for every logical input channel (x may carry pad channels in the
        middle of a concat): the input-channel axis of every weight that reads x is re-indexed"""
        phys = b.tensors[x][0] if col_map is not None else None         # (None: the builder takes the weights as they are)

        def remap(w):                                   # (Co, C_logical[, k, k]) -> (Co, C_physical[, k, k])
            if col_map is None:
                return None
            w = w.detach().float().cpu()
            out = torch.zeros((w.shape[0], phys) + tuple(w.shape[2:]))
            out[:, col_map] = w
            return out
        res = b.conv(x, self.residual[0], self.residual[1], relu=True, weight=remap(self.residual[0].weight), cin=phys)
        gate = self.se.emit(b, x, w1=remap(self.se.fc[0].weight))
        # torch.cat of the dilated branches (:191) without a copy: every branch writes its
        # channels side by side; each slice is padded to the builder's granule (16 bytes: 4 fp32 or 8 fp16 channels)
        hc = self.hdcs[0][0].out_channels
        hp = -(-hc // b.granule) * b.granule
        nd = len(self.hdcs)
        cat = b.new_tensor(hp * nd, b.tensors[x][1])
        for i, hdc in enumerate(self.hdcs):
            b.conv(x, hdc[0], hdc[1], relu=True, out=(cat, hp * i), cout_store=hp, weight=remap(hdc[0].weight), cin=phys)
        w = self.hdc_top[0].weight.detach().cpu()                      # (C, hc*nd, 1, 1)
        wp = torch.zeros((w.shape[0], hp * nd, 1, 1), dtype=w.dtype)
        for i in range(nd):
            wp[:, hp * i:hp * i + hc] = w[:, hc * i:hc * (i + 1)]
        top = b.conv(cat, self.hdc_top[0], self.hdc_top[1], relu=True, weight=wp, cin=hp * nd)
        return b.cam_combine(top, res, gate)

    def forward(self, x):
        raise RuntimeError("rtpe: ContextAwareModule runs only inside a compiled student program")


class StemHRNet(torch.nn.Module):
    """stem + layer1 of HigherHRNet (reference :206-283); same keys as the teacher's stem"""
    INPLANES = 64

    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, self.INPLANES, kernel_size=3, stride=2, padding=1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(self.INPLANES, momentum=BN_MOMENTUM)
        self.conv2 = torch.nn.Conv2d(self.INPLANES, self.INPLANES, kernel_size=3, stride=2, padding=1, bias=False)
        self.bn2 = torch.nn.BatchNorm2d(self.INPLANES, momentum=BN_MOMENTUM)
        self.relu = torch.nn.ReLU(inplace=True)
        proj = torch.nn.Sequential(torch.nn.Conv2d(64, 256, kernel_size=1, stride=1, bias=False),
                                   torch.nn.BatchNorm2d(256, momentum=BN_MOMENTUM))
        self.layer1 = torch.nn.Sequential(Bottleneck(64, 64, 1, proj), *[Bottleneck(256, 64) for _ in range(3)])

    def emit(self, b):
        t = b.stem(self.conv1, self.bn1)
        t = b.conv(t, self.conv2, self.bn2, relu=True)
        for blk in self.layer1:
            t = blk.emit(b, t)
        return t

    def load_pretrained(self, hhrnet_statedict_path, device="cpu", check=False):
        """reference :262-283: picks the stem keys (``1.`` + key) out of the teacher checkpoint"""
        hhrnet_d = torch.load(hhrnet_statedict_path, map_location=device)
        self.load_state_dict({k: hhrnet_d["1." + k] for k in self.state_dict()})
        if check:
            assert all((hhrnet_d["1." + k].to(device) == v.to(device)).all() for k, v in self.state_dict().items())

    def forward(self, x):
        raise RuntimeError("rtpe: StemHRNet runs only inside a compiled student program")


def get_pretrained_stem(hhrnet_statedict_path, device="cuda", half_precision=True):
    """reference :286-298"""
    stem = network_to_half(StemHRNet()) if half_precision else \
        torch.nn.Sequential(torch.nn.Identity(), StemHRNet())
    stem[1].load_pretrained(hhrnet_statedict_path, device, check=False)
    return stem


def _mixed_canvases(who, canvas, sizes, alt=None):
    """what every ``forward_mixed`` checks of its canvases before any GPU work: the canvas, [the ``alt`` canvas against
    it,] then the sizes -> ``sizes`` as ``check_mixed_sizes`` returns them"""
    if canvas.dim() != 4 or canvas.shape[1] != 3:
        raise ValueError("%s: expected a canvas (N,3,Hc,Wc), got %s" % (who, tuple(canvas.shape)))
    if alt is not None:
        if not torch.is_tensor(alt) or tuple(alt.shape) != tuple(canvas.shape):
            raise ValueError("%s: alt must be a canvas like the first, %s, got %s" %
                             (who, tuple(canvas.shape), tuple(alt.shape) if torch.is_tensor(alt) else type(alt).__name__))
        if alt.device != canvas.device:
            raise ValueError("%s: the canvases are on different devices (%s and %s)" % (who, canvas.device, alt.device))
    return check_mixed_sizes(sizes, canvas.shape[0], canvas.shape[2], canvas.shape[3])


class _StudentTrunk(CompiledModule):
    """what the student classes share: the trunk (the HigherHRNet stem, then ``mid_stem``) in front of a body of the class's
    own, the steps of the constructor on either side of that body, and the loading of the bundled attention weights.  The
    modules are registered in the reference's order - trunk, then body - which is the order of the state-dict keys and
    the order in which ``init_fn`` draws."""

    def _begin(self, inplanes, num_heatmaps, ae_dims, trainable_stem, bn_momentum):
        """the attributes and the trunk; the class registers its body next"""
        self.bn_momentum = bn_momentum
        self.num_heatmaps, self.ae_dims = num_heatmaps, ae_dims
        self.stem = StemHRNet()
        self.stem_out_chans = self.stem.layer1[-1].bn3.num_features
        self.trainable_stem = trainable_stem
        self.inplanes = inplanes
        mid = (self.stem_out_chans + inplanes) // 2
        m1, m2 = _cbr(self.stem_out_chans, mid, 3, bn_momentum=bn_momentum), _cbr(mid, inplanes, 3, bn_momentum=bn_momentum)
        self.mid_stem = torch.nn.Sequential(*m1, *m2)

    def _finish(self, hhrnet_statedict_path, device, half_precision, init_fn, body_half):
        """behind the body: the initialiser, the half wrapper and the pretrained weights of the stem, ``body_half``: every
        module behind the stem in fp16, then the engines and the device"""
        if init_fn is not None:
            self.apply(lambda module: init_weights(module, init_fn, 0.0))
        self.stem = network_to_half(self.stem) if half_precision else \
            torch.nn.Sequential(torch.nn.Identity(), self.stem)
        if hhrnet_statedict_path is not None:
            self.stem[1].load_pretrained(hhrnet_statedict_path, device, check=False)
        if body_half:                  # fp16 parameters, fp32 BatchNorm: fp32 checkpoints load into them as usual
            for name, module in self.named_children():
                if name != "stem":
                    BN_convert_float(module.half())
        self._init_compiled()
        self.to(device)
        self.device = device

    def _pool_cam_body(self, chans, dilations, top_chans):
        """reference :651-706 / :871-899: [AvgPool+CAM, AvgPool+CAM, CAM, 3x3 conv with bias]"""
        pool = lambda: torch.nn.AvgPool2d(kernel_size=3, stride=2, padding=1, count_include_pad=False)
        cam = lambda: ContextAwareModule(chans, hdc_dilations=dilations)
        top = torch.nn.Sequential(torch.nn.Conv2d(chans, top_chans, kernel_size=3, stride=1, dilation=1, padding=1, bias=True))
        return torch.nn.ModuleList([torch.nn.Sequential(pool(), cam()), torch.nn.Sequential(pool(), cam()),
                                    torch.nn.Sequential(cam()), top])

    def load_state_dicts(self, inpath):
        """reference :708-722 / :950-964"""
        for name in ("mid_stem", "att_lo", "att_mid", "att_hi", "att_top"):
            getattr(self, name).load_state_dict(torch.load(inpath + name + ".statedict", map_location="cpu"))
        self.invalidate()


class AttentionStudent(_StudentTrunk):
    """reference :595-771"""

    def __init__(self, hhrnet_statedict_path=None, device="cuda", inplanes=48, num_heatmaps=17, ae_dims=1,
                 half_precision=True, init_fn=torch.nn.init.kaiming_normal_, trainable_stem=False,
                 bn_momentum=0.1, body_half=False):
        """``body_half=True`` (needs ``half_precision=True``): everything behind the stem runs in fp16 storage with fp32
        accumulation too - the reference module after ``BN_convert_float(model.half())`` with the ``tofp32`` between stem and
        body removed: fp16 parameters, fp32 BatchNorm, fp16 activations, the outputs fp16 values returned as fp32."""
        if body_half and not half_precision:
            raise ValueError("rtpe: AttentionStudent(body_half=True) needs half_precision=True (the half body reads the "
                             "fp16 output of the half-wrapped stem)")
        super().__init__()
        self.body_half = bool(body_half)
        self._begin(inplanes, num_heatmaps, ae_dims, trainable_stem, bn_momentum)
        self.att_lo, self.att_mid, self.att_hi, self.att_top = self._pool_cam_body(inplanes, [1, 2, 3, 4, 5], 1)
        self.det_lo, self.det_mid, self.det_hi, self.det_top = self._pool_cam_body(inplanes, [1, 2, 3, 4], num_heatmaps + ae_dims)
        self._finish(hhrnet_statedict_path, device, half_precision, init_fn, self.body_half)

    def compile_program(self):
        """the forward of reference :724-771 as one program"""
        half = isinstance(self.stem[0], tofp16)
        body_half = getattr(self, "body_half", False)
        # half body: no cast, every op behind the stem stays fp16 (rows and concat slices of multiples of 8 channels)
        b = ProgramBuilder(f32=not half, any_size=True, granule=8 if body_half else 4)
        t = self.stem[1].emit(b)
        if half and not body_half:
            t = b.cast(t)                                   # tofp32 of the wrapped stem
        b.f32 = not body_half
        m = self.mid_stem
        t = b.conv(t, m[0], m[1], relu=True)
        stem_out = b.conv(t, m[3], m[4], relu=True)
        # human-mask (attention) head: hi + up(lo) + up(lo), :736-744
        hi = self.att_hi[0].emit(b, stem_out)
        mid = self.att_mid[1].emit(b, b.avgpool(stem_out))
        lo = self.att_lo[1].emit(b, b.avgpool(mid))
        att = b.fuse([(hi, 0), (lo, 2), (lo, 2)], relu=False)
        logits = b.conv(att, self.att_top[0], None)
        stem_out = b.sigmoid_add(logits, stem_out, out_flag=nat.F_OUT_PREDS)     # :755-756
        # keypoint head: det_hi for hi AND mid, det_lo on top of it, :759-769
        hi = self.det_hi[0].emit(b, stem_out)
        lo = self.det_lo[1].emit(b, b.avgpool(hi))
        det = b.fuse([(hi, 0), (lo, 1), (lo, 1)], relu=False)
        b.conv(det, self.det_top[0], None, out_flag=nat.F_OUT_REFINED, nhwc=False)
        return b.finish()

    def forward(self, x, out_hw=None, return_intermediate=False):
        """x (N,3,H,W) fp32 on the GPU, any H, W >= 32 -> (att (N,1,ceil(H/4),ceil(W/4)) = sigmoid mask,
        det (N,num_heatmaps+ae_dims,ceil(H/4),ceil(W/4))), both fp32 (``body_half=True``: fp16 values).  ``out_hw`` and
        ``return_intermediate`` are accepted and unused, as in the reference.

        Sizes.  As in the reference every map is ``ceil(n / 2^d)`` wide (the stride-2 convs and ``AvgPool2d(3, 2, 1)``),
        and the low-resolution terms of the two heads are brought to the stem's size with
        ``F.interpolate(mode="nearest", size=...)``'s index rule.  Inputs whose sides are both multiples of 32 run the
        tuned fast kernels (the first forward of a new (N, H, W) autotunes its launch shapes).  Any other size runs the
        general kernels - every conv on the one-workgroup-per-tile kernel, the stem on the VALU kernel - with their
        default launch shapes and is never autotuned: a stream of native-size images has hundreds of shapes.  The
        throughput at such sizes has not been measured.  Activation workspaces are cached per shape within
        ``RTPE_WS_CACHE_MB``, least recently used dropped."""
        self._check_inference(x, "AttentionStudent.forward")
        att, det = self._engine(x.device).forward(x.float(), torch.float32)
        return att, det

    def forward_mixed(self, canvas, sizes):
        """one forward over N images of different sizes: ``canvas`` (N,3,Hc,Wc) fp32 on the GPU with image n at
        ``[n, :, :h_n, :w_n]`` and ``sizes = [(h_n, w_n)]`` (``pack_mixed``) -> (att (N,1,eh,ew), det
        (N,num_heatmaps+ae_dims,eh,ew)) with eh, ew = the extents of Hc, Wc at 1/4.  Image n's region
        ``[n, :, :ceil(h_n/4), :ceil(w_n/4)]`` holds the bits of ``self(x_n[None])``; every element outside the regions is
        0.0, whatever the canvas holds outside the images (``unpack_mixed`` gives the regions).  Both bodies.

        Every kernel addresses by the canvas extents and masks by image n's own ("Mixed-size
        batches").  A mixed batch always runs the general kernels on default launch shapes and is never autotuned,
        whatever the canvas size."""
        sizes = _mixed_canvases("AttentionStudent.forward_mixed", canvas, sizes)     # (before any GPU work)
        self._check_inference(canvas, "AttentionStudent.forward_mixed")
        att, det = self._engine(canvas.device).forward_mixed(canvas.float(), sizes)
        return att, det


class AttentionStudentSteps(_StudentTrunk):
    """reference :786-1063: the student that ``distillation.py:137`` trains.  The stem features get the
    down-scaled ``alt`` image (the input in LAB or HSV, ``rtpe.dataloaders.rgb2lab``) concatenated, the attention head
    gates them (``stem_out * sigmoid(att)``), a second 5x5-stride-2 stem of the alt image is concatenated and three
    CAMs + a 3x3 conv give the heat maps.  Same constructor, attribute names (state-dict keys) and
    ``forward(x, out_hw=None, alt=None, att_divisor=None) -> (att, det)`` as the reference; one compiled program per
    ``att_divisor`` value."""
    _HALF_BODY = False          # AttentionStudentStepsHalf: the body's parameters are prepared as fp16 behind the stem

    def __init__(self, hhrnet_statedict_path=None, device="cuda", inplanes=48, num_heatmaps=17, ae_dims=1,
                 half_precision=True, init_fn=torch.nn.init.kaiming_normal_, trainable_stem=False, bn_momentum=0.1,
                 body_half=False):
        if body_half:
            raise NotImplementedError("rtpe: AttentionStudentSteps has no half body: its second-input ops (aux pack, resize, "
                                      "gate_mul, the 5x5 stem) exist in fp32 only; use body_half=False")
        super().__init__()
        if inplanes % 4:
            raise NotImplementedError("rtpe: AttentionStudentSteps needs inplanes to be a multiple of 4 (16-byte rows)")
        self._begin(inplanes, num_heatmaps, ae_dims, trainable_stem, bn_momentum)
        self._alt_planes = 50

        def c5(cin, cout):
            return [torch.nn.Conv2d(cin, cout, kernel_size=5, stride=2, dilation=1, padding=2, bias=False),
                    torch.nn.BatchNorm2d(cout, momentum=bn_momentum), torch.nn.ReLU(inplace=True)]
        self.alt_img_stem = torch.nn.Sequential(*c5(3, self._alt_planes), *c5(self._alt_planes, inplanes))
        self.att_lo, self.att_mid, self.att_hi, self.att_top = self._pool_cam_body(inplanes + 3, [1, 2, 3, 4], 1)
        self.steps = self._detection_stage()
        self._finish(hhrnet_statedict_path, device, half_precision, init_fn, self._HALF_BODY)

    def _detection_stage(self):
        """reference :901-948: three CAMs over [gated stem + alt (inplanes + 3) | alt stem (inplanes)], then 3x3"""
        c = 2 * self.inplanes + 3
        return torch.nn.Sequential(*[ContextAwareModule(c, hdc_dilations=[1, 2, 3]) for _ in range(3)],
                                   torch.nn.Conv2d(c, self.num_heatmaps + self.ae_dims, kernel_size=3, stride=1,
                                                   dilation=1, padding=1, bias=True))

    def compile_program(self, variant=None):
        """the forward of reference :966-1040 as one program (``variant`` = ("att_divisor", value)), for both bodies.  The
        half body (``_HALF_BODY``): no cast and no fp32 op behind the stem, the fp16 forms of the second-input ops, and
        every row and concat slice padded to 8 channels instead of 4 (``pad``: 16 bytes of the body's elements)"""
        att_divisor = variant[1] if variant else None
        half = isinstance(self.stem[0], tofp16)
        body_half = self._HALF_BODY
        P = self.inplanes
        b = ProgramBuilder(f32=not half, any_size=True, granule=8 if body_half else 4)
        pad = b.granule
        t = self.stem[1].emit(b)
        if half and not body_half:
            t = b.cast(t)                                       # tofp32 of the wrapped stem
        b.f32 = not body_half
        m = self.mid_stem
        t = b.conv(t, m[0], m[1], relu=True)
        # torch.cat((stem_out, alt), 1) (:1002) without a copy: [mid stem (P) | alt at 1/4 resolution (3) | 0 x (pad - 3)]
        cat1 = b.new_tensor(P + pad, b.tensors[t][1])
        b.conv(t, m[3], m[4], relu=True, out=(cat1, 0), cout_store=P)
        alt = b.aux_input(half=body_half)                       # rows of (r, g, b, 0 x (pad - 3)); half: alt.half()
        # F.interpolate(alt, (h, w), mode="bilinear"), :996-1000 (the pad channels: interpolated zeros)
        b.resize(alt, cat1, P, pad, half=body_half)
        # the second stem of the alt image (:984): two 5x5 stride-2 convs, pad (3 used) -> 50 stored as 56 -> P
        a = self.alt_img_stem
        u = b.conv(alt, a[0], a[1], relu=True)
        # attention head (:1004-1019): hi + up(lo) + up(lo), the reference's double use of lo reproduced
        hi = self.att_hi[0].emit(b, cat1)
        mid = self.att_mid[1].emit(b, b.avgpool(cat1))
        lo = self.att_lo[1].emit(b, b.avgpool(mid))
        att = b.fuse([(hi, 0), (lo, 2), (lo, 2)], relu=False)
        logits = b.conv(att, self.att_top[0], None)
        # stem_out * att, then torch.cat((stem_out, alt_stem_out), 1) (:1040-1042):
        # [gated (P + 3) | 0 x (pad - 3) | alt stem (P)]
        cat2 = b.new_tensor(2 * P + pad, b.tensors[cat1][1])
        b.gate_mul(logits, cat1, cat2, P + pad, att_divisor, out_flag=nat.F_OUT_PREDS, half=body_half)
        b.conv(u, a[3], a[4], relu=True, out=(cat2, P + pad), cout_store=P)
        col_map = list(range(P + 3)) + list(range(P + pad, 2 * P + pad))
        x = self.steps[0].emit(b, cat2, col_map=col_map)
        x = self.steps[1].emit(b, x)
        x = self.steps[2].emit(b, x)
        b.conv(x, self.steps[3], None, out_flag=nat.F_OUT_REFINED, nhwc=False)
        return b.finish()

    def forward_mixed(self, canvas, sizes, alt=None, att_divisor=None):
        """one forward over N images of different sizes: ``canvas`` and ``alt`` (N,3,Hc,Wc) fp32 on the GPU with image n
        (and the image in the alternative colour space) at ``[n, :, :h_n, :w_n]`` of both, ``sizes = [(h_n, w_n)]``
        (``pack_mixed(images)``, ``pack_mixed(alts, canvas_hw=canvas.shape[2:])``) -> (att, det) canvases as
        ``AttentionStudent.forward_mixed`` returns them: image n's region ``[n, :, :ceil(h_n/4), :ceil(w_n/4)]`` holds the
        bits of ``self(x_n[None], alt=alt_n[None], att_divisor=att_divisor)``, every other element is 0.0 whatever either
        canvas holds outside the images.  One compiled program per ``att_divisor`` value, as for ``forward``.

        The resize of ``alt`` takes image n's own scale, clamp and extents from the extent table, every conv masks by
        them ("Mixed-size batches: the Steps student").  General kernels on default launch shapes,
        never autotuned."""
        who = "AttentionStudentSteps.forward_mixed"
        if alt is None:                   # (as forward's "alt is expected")
            raise NotImplementedError("rtpe: %s needs the second input: alt=, the canvas of the images in the alternative "
                                      "colour space (pack_mixed(alts, canvas_hw=canvas.shape[2:]))" % who)
        sizes = _mixed_canvases(who, canvas, sizes, alt)     # (before any GPU work)
        self._check_inference(canvas, who)
        eng = self._engine(canvas.device, ("att_divisor", None if att_divisor is None else float(att_divisor)))
        att, det = eng.forward_mixed(canvas.float(), sizes, aux=alt.float())
        return att, det

    def forward(self, x, out_hw=None, alt=None, att_divisor=None):
        """x (N,3,H,W) fp32 on the GPU (any H, W >= 32), alt (N,3,H,W) fp32: the image in the alternative
        colour space -> (att (N,1,ceil(H/4),ceil(W/4)) = sigmoid mask, det (N,num_heatmaps+ae_dims,ceil(H/4),ceil(W/4))),
        both fp32.  Sizes, kernels and tuning: as for ``AttentionStudent.forward`` - multiples of 32 run the tuned fast
        kernels; any other size runs the general kernels on default launch shapes, is never autotuned, and its
        throughput has not been measured.  ``AttentionStudentStepsHalf``: ``alt`` stays an fp32 tensor and is rounded to
        fp16 as it is packed; both outputs are fp32 tensors that hold fp16 values."""
        self._check_inference(x, type(self).__name__ + ".forward")
        if alt is None:
            raise NotImplementedError("ATM alt is expected")        # reference :993-994
        eng = self._engine(x.device, ("att_divisor", None if att_divisor is None else float(att_divisor)))
        att, det = eng.forward(x.float(), torch.float32, aux=alt.to(x.device).float())
        return att, det


class AttentionStudentStepsHalf(AttentionStudentSteps):
    """``AttentionStudentSteps`` end to end in fp16: the reference module after ``BN_convert_float(model.half())`` with the
    ``tofp32`` between stem and body removed and ``alt.half()`` as its second input - fp16 parameters, fp32 BatchNorm, fp16
    activations, fp32 accumulation, the outputs fp16 values returned as fp32 ("Half body: the Steps
    student").  Same positional arguments as ``AttentionStudentSteps`` without ``body_half``, same attribute names and
    state-dict keys; fp32 checkpoints load as usual and the BatchNorms keep their fp32 values.  Every row, offset and concat
    slice of the compiled program is a multiple of 8 channels, so ``inplanes`` must be one."""
    _HALF_BODY = True

    def __init__(self, hhrnet_statedict_path=None, device="cuda", inplanes=48, num_heatmaps=17, ae_dims=1,
                 half_precision=True, init_fn=torch.nn.init.kaiming_normal_, trainable_stem=False, bn_momentum=0.1):
        if not half_precision:
            raise ValueError("rtpe: AttentionStudentStepsHalf needs half_precision=True (the half body reads the fp16 output of "
                             "the half-wrapped stem)")
        if inplanes <= 0 or inplanes % 8:
            raise ValueError("rtpe: AttentionStudentStepsHalf needs inplanes to be a multiple of 8 (16-byte rows of fp16 "
                             "channels), got %r" % (inplanes,))
        super().__init__(hhrnet_statedict_path, device, inplanes, num_heatmaps, ae_dims, True, init_fn, trainable_stem,
                         bn_momentum)

    def forward_mixed(self, canvas, sizes, alt=None, att_divisor=None):
        """not built: refused before any GPU work"""
        self.refuse_mixed()

    def refuse_mixed(self):
        """what ``StudentPipeline.call_mixed`` / ``stream_mixed`` ask before they pack a batch"""
        raise NotImplementedError("rtpe: AttentionStudentStepsHalf.forward_mixed: the masked fp16 forms of the second-input ops "
                                  "(aux pack, resize, gate_mul) do not exist yet; run a mixed-size batch on "
                                  "AttentionStudentSteps, or this model one size per batch")
