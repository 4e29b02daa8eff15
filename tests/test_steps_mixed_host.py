"""CPU tests of the mixed-size batch of AttentionStudentSteps (include/rtpe_hip_mixed_aux.h,
AttentionStudentSteps.forward_mixed, StudentPipeline.call_mixed(alt=...)): the ABI of the new entry, the refusals that come
before any GPU work, the cut of ``mixed_batches(alts=...)`` - and the premise of the resize's mixed form: the bilinear
resize of the second input at the canvas' scale is another function than the resize of the image alone."""
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_student_mixed_host as M
import test_student_sizes_host as S
from oracle import student_ref, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(min(16, torch.get_num_threads()))

# the whole-network batch of tests/test_steps_mixed_gpu.py: the fixture's two cases first (S.STEPS_CASES: image and alt
# seeds 111 / 112 and 113 / 114), then two images with multiple-of-32 sides
NET_SIZES = M.NET_SIZES
NET_SEEDS = [(111, 112), (113, 114), (135, 136), (137, 138)]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


# --------------------------------------------------------------------------- #
# ABI
# --------------------------------------------------------------------------- #
def test_the_new_entry_is_declared_in_its_own_header_and_resolves(built):
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, hdr = strip("rtpe_hip.h"), strip("rtpe_hip_mixed_aux.h")
    assert len(re.findall(r'#include "rtpe_hip_mixed_aux.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"rtpe_hrnet_forward_mixed_aux"} == set(built.EXPORTS_MIXAUX)
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR, built.EXPORTS_RECORDS,
             built.EXPORTS_TAGMEAN, built.EXPORTS_NOPROJ, built.EXPORTS_ANYSIZE, built.EXPORTS_MIXED, built.EXPORTS_MIXDEC,
             built.EXPORTS_TRACE)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2, 6, 5, 4, 4, 4, 2]      # no change to the existing tables
    for table in older:
        assert not declared & set(table)
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "rtpe_hip_mixed_aux.h":
            assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", strip(name))), name
    lib = built.lib()
    sig = built._SIGS_MIXAUX["rtpe_hrnet_forward_mixed_aux"][1]
    assert lib.rtpe_hrnet_forward_mixed_aux.argtypes == sig
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4
    # the arguments of rtpe_hrnet_forward_mixed plus the second input, where rtpe_hrnet_forward_aux has it
    fm, fa = built._SIGS_MIXED["rtpe_hrnet_forward_mixed"][1], built._SIGS["rtpe_hrnet_forward_aux"][1]
    assert sig[:3] == fm[:3] and sig[4:] == fm[3:] and len(sig) == len(fm) + 1 and sig[:4] == fa[:4]
    # the comment block of rtpe_hip_mixed.h says where such a program goes
    assert "rtpe_hip_mixed_aux.h" in open(os.path.join(ROOT, "include", "rtpe_hip_mixed.h")).read()


def test_the_new_entry_refuses_null_arguments_without_a_gpu(built):
    import ctypes
    lib = built.lib()
    flat = (ctypes.c_int32 * 2)(32, 32)
    one = ctypes.c_void_p(16)              # (never dereferenced: every call below is refused at its argument checks)
    assert lib.rtpe_hrnet_forward_mixed_aux(None, None, 2, None, 1, 64, 64, flat, None, 12, None, None, 2, None, 0, None, 0) == -1
    assert b"second input is null" in lib.rtpe_last_error_string()
    assert lib.rtpe_hrnet_forward_mixed_aux(None, None, 2, one, 1, 64, 64, flat, None, 12, None, None, 2, None, 0, None, 0) == -1
    assert b"null argument" in lib.rtpe_last_error_string()


# --------------------------------------------------------------------------- #
# refusals before any GPU work
# --------------------------------------------------------------------------- #
def test_steps_forward_mixed_checks_everything_before_any_gpu_work(monkeypatch):
    from rtpe.students import AttentionStudent, AttentionStudentSteps
    from rtpe.third_party.pose_higher_hrnet import CompiledModule, Engine

    def no_gpu(*a, **k):
        raise AssertionError("GPU work")
    monkeypatch.setattr(CompiledModule, "_engine", no_gpu)
    steps = AttentionStudentSteps(None, "cpu", inplanes=48).eval()
    canvas, alt = torch.zeros(3, 3, 64, 47), torch.zeros(3, 3, 64, 47)
    with pytest.raises(NotImplementedError, match="second input"):          # as forward's "alt is expected"
        steps.forward_mixed(canvas, M.OP_SIZES)
    with pytest.raises(NotImplementedError, match="second input"):
        steps.forward_mixed(canvas, M.OP_SIZES, att_divisor=20.0)
    for sizes, msg in (([(31, 47), (47, 33), (64, 32)], "at least 32"), ([(33, 47), (47, 33), (65, 32)], "larger than"),
                       ([(33, 48), (47, 33), (64, 32)], "larger than"), (M.OP_SIZES[:2], "2 sizes for a canvas of 3"), ([1, 2, 3], "pairs")):
        with pytest.raises(ValueError, match=msg):
            steps.forward_mixed(canvas, sizes, alt=alt)
    with pytest.raises(ValueError, match="canvas"):
        steps.forward_mixed(canvas[0], M.OP_SIZES, alt=alt[0])
    for bad in (alt[:2], alt[:, :, :63], alt[:, :, :, :46], alt[:, :2], [alt]):
        with pytest.raises(ValueError, match="alt must be a canvas like the first"):
            steps.forward_mixed(canvas, M.OP_SIZES, alt=bad)
    with pytest.raises(RuntimeError, match="HIP path only"):               # good arguments: the next stop is the device check
        steps.forward_mixed(canvas, M.OP_SIZES, alt=alt)
    with pytest.raises(RuntimeError, match="HIP path only"):
        steps.forward_mixed(canvas, M.OP_SIZES, alt, 20.0)                 # (positional, as the contract writes it)
    # the executor's own checks, before anything is allocated
    dev = torch.device("cuda", 0)
    eng = types.SimpleNamespace(program=steps.compile_program(("att_divisor", None)), device=dev)
    assert eng.program.has_aux and eng.program.any_size
    with pytest.raises(ValueError, match="second input"):
        Engine._io_mixed(eng, canvas, M.OP_SIZES)
    with pytest.raises(ValueError, match="at least 32"):
        Engine._io_mixed(eng, canvas, [(31, 47), (47, 33), (64, 32)], alt)
    with pytest.raises(RuntimeError, match="executor lives on"):            # the first canvas is looked at first
        Engine._io_mixed(eng, canvas, M.OP_SIZES, alt)
    on_cpu = types.SimpleNamespace(program=eng.program, device=canvas.device)      # (a stand-in: the device check passes)
    for bad in (alt[:2], alt[:, :, :63], alt.double(), alt.half()):               # shape, dtype
        with pytest.raises(ValueError, match="second input as a float32 canvas"):
            Engine._io_mixed(on_cpu, _cuda_like(canvas), M.OP_SIZES, bad)
    plain = types.SimpleNamespace(program=AttentionStudent(None, "cpu", inplanes=48).compile_program(), device=dev)
    with pytest.raises(ValueError, match="has no second input"):
        Engine._io_mixed(plain, canvas, M.OP_SIZES, alt)


class _CudaLike(torch.Tensor):
    """a CPU tensor that says it is on the GPU: ``Engine._io_mixed`` reaches its checks of the second canvas without one"""
    is_cuda = True


def _cuda_like(t):
    return t.as_subclass(_CudaLike)


class _NeedsAlt(torch.nn.Module):
    def forward(self, x, alt=None):
        raise AssertionError("GPU work")

    def forward_mixed(self, canvas, sizes, alt=None, att_divisor=None):
        raise AssertionError("GPU work")


class _NoAlt(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("GPU work")

    def forward_mixed(self, canvas, sizes):
        raise AssertionError("GPU work")


def _pipe(model):
    from rtpe.engine import StudentPipeline
    from test_student_pipeline_host import _parser
    pipe = StudentPipeline.__new__(StudentPipeline)         # (the constructor moves the model to a GPU)
    pipe.model, pipe.parser = model, _parser()
    pipe.flip_test, pipe.scale_factors, pipe.ags = False, None, False
    pipe.device = torch.device("cpu")
    return pipe


def test_student_pipeline_checks_alt_before_the_forward():
    from rtpe.students import pack_mixed
    ims, alts = M._images(M.OP_SIZES), M._images(M.OP_SIZES, seed=6)
    pipe = _pipe(_NeedsAlt())
    with pytest.raises(ValueError, match="needs the second input"):
        pipe.call_mixed(ims)
    with pytest.raises(ValueError, match="2 alt images for 3 images"):
        pipe.call_mixed(ims, alt=alts[:2])
    with pytest.raises(ValueError, match=r"alt image 1 must be a \(3, 47, 33\) tensor"):
        pipe.call_mixed(ims, alt=[alts[0], alts[0], alts[2]])
    with pytest.raises(ValueError, match="alt image 0"):
        pipe.call_mixed(ims, alt=[alts[0][None], alts[1], alts[2]])
    with pytest.raises(ValueError, match="at least 32"):                  # the images' own refusals come first, as ever
        pipe.call_mixed([torch.zeros(3, 31, 40)], alt=[torch.zeros(3, 31, 40)])
    with pytest.raises(ValueError, match="2 image ids for 3 images"):
        pipe.call_mixed(ims, image_ids=[1, 2], alt=alts)
    with pytest.raises(AssertionError, match="GPU work"):                 # good arguments reach the forward
        pipe.call_mixed(ims, alt=alts)
    # the batches of stream_mixed: (images, alts) pairs and (canvas, sizes, alt_canvas) triples
    canvas, sizes = pack_mixed(ims)
    alt_canvas, _ = pack_mixed(alts, canvas_hw=canvas.shape[2:])
    assert pipe._is_mixed((ims, alts)) and pipe._is_mixed((canvas, sizes, alt_canvas)) and pipe._is_mixed([ims, alts])
    assert not pipe._is_mixed([canvas, canvas, canvas]) and not pipe._is_mixed((canvas, None, alt_canvas))
    batch, hw = pipe._mixed_begin((ims, alts))
    assert hw == M.OP_SIZES and len(batch) == 3 and torch.equal(batch[0], canvas) and torch.equal(batch[2], alt_canvas)
    batch, hw = pipe._mixed_begin((canvas, sizes, alt_canvas))
    assert hw == M.OP_SIZES and batch[0] is canvas and batch[2] is alt_canvas
    for bad, msg in ((ims, "needs the second input"), ((canvas, sizes), "needs the second input"),
                     ((ims, alts[:2]), "2 alt images"), ((canvas, sizes, alt_canvas[:2]), "alt canvas"),
                     ((canvas, sizes, alt_canvas[:, :, :, :40]), "alt canvas"), ((canvas, sizes[:2], alt_canvas), "2 sizes")):
        with pytest.raises(ValueError, match=msg):
            pipe._mixed_begin(bad)
    with pytest.raises(ValueError, match="call_mixed"):                   # stream() and __call__ keep refusing every mixed form
        pipe((ims, alts))
    with pytest.raises(ValueError, match="call_mixed"):
        pipe._decode_hw(None, (canvas, sizes, alt_canvas))
    # a model without a second input: what existing callers pass keeps its behaviour; alt is refused, not dropped
    plain = _pipe(_NoAlt())
    with pytest.raises(AssertionError, match="GPU work"):
        plain.call_mixed(ims)
    with pytest.raises(ValueError, match="takes no second input"):
        plain.call_mixed(ims, alt=alts)
    with pytest.raises(ValueError, match="takes no second input"):
        plain._mixed_begin((ims, alts))
    with pytest.raises(ValueError, match="takes no second input"):
        plain._mixed_begin((canvas, sizes, alt_canvas))
    assert len(plain._mixed_begin(ims)[0]) == 2 and len(plain._mixed_begin((canvas, sizes))[0]) == 2


# --------------------------------------------------------------------------- #
# mixed_batches(alts=...)
# --------------------------------------------------------------------------- #
def test_mixed_batches_cuts_the_alts_in_the_order_of_the_images():
    from rtpe.engine import StudentPipeline
    g = torch.Generator().manual_seed(9)
    sizes = [(int(h), int(w)) for h, w in torch.randint(32, 90, (11, 2), generator=g).tolist()]
    ims = [types.SimpleNamespace(shape=(3, h, w), tag=i) for i, (h, w) in enumerate(sizes)]
    alts = [types.SimpleNamespace(shape=(3, h, w), tag=100 + i) for i, (h, w) in enumerate(sizes)]
    plain, _ = StudentPipeline.mixed_batches(ims, batch_size=4)
    batches, restore = StudentPipeline.mixed_batches(ims, batch_size=4, alts=alts)
    assert [len(b) for b in plain] == [4, 4, 3] and len(batches) == 3
    for b, p in zip(batches, plain):
        assert isinstance(b, tuple) and len(b) == 2
        assert [i.tag for i in b[0]] == [i.tag for i in p]                  # the same cut as without alts ...
        assert [a.tag for a in b[1]] == [100 + i.tag for i in b[0]]         # ... and every alt with its image
    areas = [i.shape[1] * i.shape[2] for b in batches for i in b[0]]
    assert areas == sorted(areas)
    back = restore([[i.tag for i in b[0]] for b in batches])
    assert back == list(range(11))
    with pytest.raises(ValueError, match="10 alts for 11 images"):
        StudentPipeline.mixed_batches(ims, batch_size=4, alts=alts[:10])
    with pytest.raises(ValueError, match="do not go with"):
        restore([[0] * 4, [0] * 4])
    with pytest.raises(ValueError, match="at least 1"):
        StudentPipeline.mixed_batches(ims, batch_size=0, alts=alts)


# --------------------------------------------------------------------------- #
# the premise: the resize has to know the image's own size
# --------------------------------------------------------------------------- #
def test_the_resize_at_the_canvas_scale_is_not_the_resize_of_the_image(golden_dir):
    """the 33 x 47 ``alt`` image (S.STEPS_CASES) zero-padded into a 64 x 47 canvas: ``F.interpolate`` of the canvas to its
    16 x 12 map, cropped to the image's 9 x 12, against ``F.interpolate`` of the image alone to 9 x 12.  The scale along H
    is 64 / 16 = 4.0 for the canvas and 33 / 9 = 3.667 for the image: every tap and weight moves.  And the whole student
    (the oracle) on the padded pair differs inside the image's region by far more than the students' bound."""
    name, n, h, w, seed, alt_seed, div = S.STEPS_CASES[0]
    assert (h, w) == (33, 47)
    x, alt = synth.make_images(n, h, w, seed=seed), S.steps_alt(n, h, w, alt_seed)
    canvas_alt = torch.zeros(1, 3, 64, 47)
    canvas_alt[:, :, :h, :w] = alt
    alone = F.interpolate(alt, (9, 12), mode="bilinear")
    padded = F.interpolate(canvas_alt, (16, 12), mode="bilinear")[:, :, :9, :12]
    diff = (padded - alone).abs()
    print("alt resized at the canvas scale: differs by %.3f from the image's own resize (range %.1f), %.0f %% of the elements "
          "by more than 1e-3" % (float(diff.max()), float(alone.max() - alone.min()), 100 * float((diff > 1e-3).float().mean())))
    assert float(diff.max()) > 1.0 and float((diff > 1e-3).float().mean()) > 0.9
    # along W the extents agree with the canvas' (47 -> 12 both): only the rows move
    cols = F.interpolate(canvas_alt[:, :, :h], (9, 12), mode="bilinear")
    assert torch.equal(cols, alone)
    sd = S.student_sd(golden_dir, "steps")
    att0, det0 = [t.numpy() for t in student_ref.student_steps_forward(sd, x, alt, div, half_stem=True)]
    assert det0.shape == (1, 18, 9, 12)
    canvas_x = torch.zeros(1, 3, 64, 47)
    canvas_x[:, :, :h, :w] = x
    att, det = [t.numpy() for t in student_ref.student_steps_forward(sd, canvas_x, canvas_alt, div, half_stem=True)]
    d = np.abs(det[:, :, :9, :12] - det0)
    bound = 1e-3 * max(1.0, float(np.abs(det0).max()))
    print("steps48 on the zero-padded pair: det differs by %.3f inside the image (range %.2f), %.0f %% of the elements by more "
          "than the bound %.1e; att by %.1e" % (d.max(), np.ptp(det0), 100 * (d > bound).mean(), bound,
                                               np.abs(att[:, :, :9, :12] - att0).max()))
    assert d.max() > 100 * bound and (d > bound).mean() > 0.5
    with pytest.raises(AssertionError):
        S.within((att[:, :, :9, :12], det[:, :, :9, :12]), (att0, det0), "padded vs alone")
