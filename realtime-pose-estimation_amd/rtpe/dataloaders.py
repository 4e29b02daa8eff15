"""The one piece of the reference's ``rtpe/dataloaders.py`` that sits next to the accelerated path: the
alternative colour space of ``CocoDistillationDatasetAugmented2`` (:314-375), which feeds ``AttentionStudentSteps``
its ``alt`` input.  The reference calls ``skimage.color.rgb2lab`` / ``rgb2hsv`` on the ToTensor'd image on the CPU;
here one HIP pass (``rtpe_rgb_to_alt``) does it for a batch on the GPU.  The datasets themselves (COCO I/O,
pycocotools scoring) are out of scope.

``HWHeatmapGenerator`` (:30-79), which turns labelled keypoints into Gaussian ground-truth maps, runs on the GPU as well:
``batch`` for the people of a whole batch (``rtpe.distill.JointTable``), ``__call__`` for one image with a numpy result."""
import ctypes

import torch

from . import _native as nat


def _convert(img, mode):
    t = img if torch.is_tensor(img) else torch.as_tensor(img)
    nat.require_gpu(t, "rgb2lab / rgb2hsv")
    if t.dtype != torch.float32 or t.dim() not in (3, 4) or t.shape[-3] != 3:
        raise TypeError("expected a float32 (3,H,W) or (N,3,H,W) RGB tensor in [0, 1]")
    x = t.contiguous().view((-1, 3) + tuple(t.shape[-2:]))
    out = torch.empty_like(x)
    with nat.on_device(x):
        nat.check(nat.lib().rtpe_rgb_to_alt(ctypes.c_void_p(x.data_ptr()), x.shape[0], x.shape[2], x.shape[3], mode,
                                            ctypes.c_void_p(out.data_ptr()), nat.stream_ptr(x.device)))
    return out.view(t.shape)


def rgb2lab(img):
    """(3,H,W) / (N,3,H,W) float32 RGB in [0,1] on the GPU -> CIE-LAB (D65), L in [0,100]; what the reference gets
    from ``skimage.color.rgb2lab`` + ``to_tensor`` (dataloaders.py:352-356)"""
    return _convert(img, 0)


def rgb2hsv(img):
    """-> HSV, all three in [0,1] (``skimage.color.rgb2hsv``)"""
    return _convert(img, 1)


def alt_colorspace(img, alt_colorspace="LAB"):
    """``colorspace_fn`` of CocoDistillationDatasetAugmented2 (:337-343)"""
    if alt_colorspace == "LAB":
        return rgb2lab(img)
    if alt_colorspace == "HSV":
        return rgb2hsv(img)
    raise NotImplementedError("Unknown color space {}".format(alt_colorspace))


class HWHeatmapGenerator:
    """per-joint ground-truth maps: every labelled keypoint (v > 0, inside the image) becomes a Gaussian patch of
    ``stddev_pixels`` around its truncated position, patches combine by maximum (csrc/distill.hip, DESIGN.md section 4,
    "Distillation targets and losses").  ``g`` is the reference's float64 patch table, built by numpy on the host."""

    def __init__(self, num_joints=17, stddev_pixels=2.0):
        from . import distill
        assert stddev_pixels > 0, "stddev_pixels must be positive"
        self.num_joints = num_joints
        self.sigma = stddev_pixels
        self.g = distill.patch_table(stddev_pixels)

    def batch(self, table, out_shape_hw):
        """(N, J, H, W) float32 CUDA tensor for a ``JointTable`` that was moved to the device: one launch"""
        from . import distill
        if table.num_joints != self.num_joints:
            raise ValueError("HWHeatmapGenerator: a table of %d joints for a generator of %d"
                             % (table.num_joints, self.num_joints))
        return distill.gt_heatmaps(table, out_shape_hw, self.sigma)

    def __call__(self, joints, out_shape_hw):
        """the reference's call: ``joints`` (P, J, 3) of one image -> (J, H, W) float32 numpy array; computed on the
        current GPU and read back (there is no CPU path)"""
        from . import distill
        if not torch.cuda.is_available():
            raise RuntimeError("rtpe: HWHeatmapGenerator runs on the MI355X HIP path only and found no GPU (there is "
                               "deliberately no CPU fallback in the product path)")
        table = distill.JointTable([joints], self.num_joints).to("cuda")
        return self.batch(table, out_shape_hw)[0].cpu().numpy()
