"""CPU tests of the mixed-size batch of the students (include/rtpe_hip_mixed.h, rtpe.students.pack_mixed /
AttentionStudent.forward_mixed, StudentPipeline.call_mixed): the extent table, the canvas layout, the ABI of the new entries,
the refusals that come before any GPU work - and the premise of the feature: zero-padding an image to a larger canvas
changes the student's answer inside the image, so the kernels have to mask.  The image sets of
tests/test_student_mixed_gpu.py live here."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import test_student_sizes_host as S
from oracle import student_ref, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(min(16, torch.get_num_threads()))

# the per-op image sets of the GPU tests: an odd side on both axes, one image with multiple-of-32 sides; in the first canvas
# every image reaches one canvas edge, in the second none does and a whole tile row and column lie outside every image
OP_SIZES = [(33, 47), (47, 33), (64, 32)]
OP_CANVASES = [(64, 47), (72, 80)]
# the whole-network batch: fixture images first (student_sizes.npz: s100_33x47 image 0, s100_100x140)
NET_SIZES = [(33, 47), (100, 140), (64, 96), (96, 64)]
NET_SEEDS = [101, 102, 131, 132]
NEW_SYMBOLS = {"rtpe_mixed_table_ints", "rtpe_mixed_table_fill", "rtpe_hrnet_mixed_workspace_bytes", "rtpe_hrnet_forward_mixed"}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


def _fill(lib, sizes, Hc, Wc, n_ints=None):
    N = len(sizes)
    flat = (ctypes.c_int32 * (2 * N))(*[v for hw in sizes for v in hw])
    n = ctypes.c_int32()
    assert lib.rtpe_mixed_table_ints(N, ctypes.byref(n)) == 0 and n.value == 12 * N
    table = (ctypes.c_int32 * n.value)(*([-7] * n.value))
    rc = lib.rtpe_mixed_table_fill(flat, N, Hc, Wc, table, n.value if n_ints is None else n_ints)
    return rc, np.array(list(table), np.int64).reshape(6, N, 2)


# --------------------------------------------------------------------------- #
# extent table
# --------------------------------------------------------------------------- #
def test_extent_table_holds_the_extent_of_every_image_at_every_level(built):
    """row d = N pairs (extent(h_n, d), extent(w_n, d)): one pointer per level; sizes 32 .. 700"""
    lib = built.lib()
    assert built.MIXED_LEVELS == 6
    hs = list(range(32, 701))
    sizes = [(h, hs[(7 * i + 3) % len(hs)]) for i, h in enumerate(hs)]        # every side value on both axes
    rc, t = _fill(lib, sizes, 700, 700)
    assert rc == 0
    for d in range(6):
        want = np.array([[built.extent(h, d), built.extent(w, d)] for h, w in sizes])
        assert np.array_equal(t[d], want), d
        assert np.array_equal(want, -(-np.array(sizes) // (1 << d)))                 # the ceil chain at every size >= 32
    rc, t = _fill(lib, OP_SIZES, 64, 47)
    assert rc == 0 and t[2].tolist() == [[9, 12], [12, 9], [16, 8]] and t[5].tolist() == [[2, 2], [2, 2], [2, 1]]


def test_extent_table_refusals(built):
    lib = built.lib()
    for sizes, canvas, msg in (([(31, 47)], (64, 64), b"at least 32"), ([(47, 31)], (64, 64), b"at least 32"),
                               ([(33, 47), (65, 40)], (64, 64), b"larger than"), ([(33, 47), (40, 65)], (64, 64), b"larger than"),
                               ([(32, 32)], (31, 64), b"canvas")):
        rc, t = _fill(lib, sizes, *canvas)
        assert rc == -1 and msg in lib.rtpe_last_error_string(), (sizes, lib.rtpe_last_error_string())
        assert (t == -7).all()                                  # refused before anything was written
    rc, t = _fill(lib, OP_SIZES, 64, 47, n_ints=35)
    assert rc == -1 and (t == -7).all()
    n = ctypes.c_int32()
    assert lib.rtpe_mixed_table_ints(0, ctypes.byref(n)) == -1 and lib.rtpe_mixed_table_ints(3, None) == -1
    flat = (ctypes.c_int32 * 2)(32, 32)
    assert lib.rtpe_mixed_table_fill(None, 1, 64, 64, (ctypes.c_int32 * 12)(), 12) == -1
    assert lib.rtpe_mixed_table_fill(flat, 1, 64, 64, None, 12) == -1
    # the forward and its workspace size refuse a null handle before anything else
    nb = ctypes.c_size_t()
    assert lib.rtpe_hrnet_mixed_workspace_bytes(None, 1, 64, 64, ctypes.byref(nb)) == -1
    assert lib.rtpe_hrnet_forward_mixed(None, None, 2, 1, 64, 64, flat, None, 12, None, None, 2, None, 0, None, 0) == -1


# --------------------------------------------------------------------------- #
# ABI
# --------------------------------------------------------------------------- #
def test_mixed_symbols_are_declared_in_their_header_and_resolve(built):
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, hdr = strip("rtpe_hip.h"), strip("rtpe_hip_mixed.h")
    assert len(re.findall(r'#include "rtpe_hip_mixed.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", hdr))
    assert declared == NEW_SYMBOLS == set(built.EXPORTS_MIXED)
    assert re.search(r"#define\s+RTPE_MIXED_LEVELS\s+6\b", hdr)
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR,
             built.EXPORTS_RECORDS, built.EXPORTS_TAGMEAN, built.EXPORTS_NOPROJ, built.EXPORTS_ANYSIZE)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2, 6, 5, 4]        # no change to the existing tables
    for table in older:
        assert not declared & set(table)
    assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", main))
    lib = built.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == built._SIGS_MIXED[name][1], name
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4
    # the arguments of rtpe_hrnet_forward_flags, plus the sizes and the pinned block of the table
    ff, fm = built._SIGS["rtpe_hrnet_forward_flags"][1], built._SIGS_MIXED["rtpe_hrnet_forward_mixed"][1]
    assert fm[:6] == ff[:6] and fm[9:] == ff[6:] and len(fm) == len(ff) + 3


# --------------------------------------------------------------------------- #
# pack_mixed / unpack_mixed
# --------------------------------------------------------------------------- #
def _images(sizes, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(3, h, w, generator=g) + 0.5 for h, w in sizes]


def test_pack_mixed_lays_every_image_at_the_origin_of_its_plane_and_zeros_elsewhere():
    from rtpe.students import pack_mixed, unpack_mixed
    ims = _images(OP_SIZES)
    canvas, sizes = pack_mixed(ims)
    assert canvas.shape == (3, 3, 64, 47) and canvas.dtype == torch.float32 and sizes == OP_SIZES
    for n, (im, (h, w)) in enumerate(zip(ims, sizes)):
        assert torch.equal(canvas[n, :, :h, :w], im)
        rest = canvas[n].clone()
        rest[:, :h, :w] = 0
        assert not rest.any() and (canvas[n, :, :h, :w] >= 0.5).all()
    big, sizes2 = pack_mixed([im.double() for im in ims], canvas_hw=(72, 80))
    assert big.shape == (3, 3, 72, 80) and big.dtype == torch.float32 and sizes2 == OP_SIZES
    assert torch.equal(big[:, :, :64, :47], canvas) and not big[:, :, 64:].any() and not big[:, :, :, 47:].any()
    # the regions of the output canvases: views, ceil(h / 4) x ceil(w / 4)
    att, det = torch.rand(3, 1, 18, 20), torch.rand(3, 18, 18, 20)
    parts = unpack_mixed(att, det, OP_SIZES)
    assert [tuple(a.shape) for a, _ in parts] == [(1, 9, 12), (1, 12, 9), (1, 16, 8)]
    for n, (a, d) in enumerate(parts):
        assert d.shape == (18,) + tuple(a.shape[1:]) and a.data_ptr() == att[n].data_ptr() and d.data_ptr() == det[n].data_ptr()
        assert torch.equal(d, det[n, :, :a.shape[1], :a.shape[2]])


def test_pack_mixed_refusals():
    from rtpe.students import pack_mixed, unpack_mixed
    with pytest.raises(ValueError, match="no images"):
        pack_mixed([])
    with pytest.raises(ValueError, match=r"\(3, h, w\)"):
        pack_mixed([torch.zeros(1, 3, 40, 40)])
    with pytest.raises(ValueError, match="at least 32"):
        pack_mixed([torch.zeros(3, 40, 40), torch.zeros(3, 31, 40)])
    with pytest.raises(ValueError, match="does not hold"):
        pack_mixed(_images(OP_SIZES), canvas_hw=(64, 46))
    with pytest.raises(ValueError, match="2 sizes for a canvas of 3"):
        unpack_mixed(torch.zeros(3, 1, 16, 12), torch.zeros(3, 18, 16, 12), OP_SIZES[:2])


# --------------------------------------------------------------------------- #
# refusals before any GPU work
# --------------------------------------------------------------------------- #
def test_forward_mixed_refuses_bad_sizes_a_teacher_and_the_steps_student_before_any_gpu_work(monkeypatch):
    from rtpe.students import AttentionStudent, AttentionStudentSteps
    from rtpe.third_party.pose_higher_hrnet import CompiledModule, Engine, PoseHigherResolutionNet

    def no_gpu(*a, **k):
        raise AssertionError("GPU work")
    monkeypatch.setattr(CompiledModule, "_engine", no_gpu)
    canvas = torch.zeros(3, 3, 64, 47)
    for half in (False, True):
        stu = AttentionStudent(None, "cpu", inplanes=48, body_half=half).eval()
        for sizes, msg in (([(31, 47), (47, 33), (64, 32)], "at least 32"), ([(33, 47), (47, 31), (64, 32)], "at least 32"),
                           ([(33, 47), (47, 33), (65, 32)], "larger than"), ([(33, 48), (47, 33), (64, 32)], "larger than"),
                           (OP_SIZES[:2], "2 sizes for a canvas of 3"), (OP_SIZES + [(32, 32)], "4 sizes"), ([1, 2, 3], "pairs")):
            with pytest.raises(ValueError, match=msg):
                stu.forward_mixed(canvas, sizes)
        with pytest.raises(ValueError, match="canvas"):
            stu.forward_mixed(canvas[0], OP_SIZES)
        with pytest.raises(RuntimeError, match="HIP path only"):            # good sizes: the next stop is the device check
            stu.forward_mixed(canvas, OP_SIZES)
    steps = AttentionStudentSteps(None, "cpu", inplanes=48).eval()
    with pytest.raises(NotImplementedError, match="second input"):
        steps.forward_mixed(canvas, OP_SIZES)
    # a program without any_size (the teacher) is refused by the executor's own check, before anything is allocated
    teacher = types.SimpleNamespace(program=PoseHigherResolutionNet().eval().compile_program(), device=torch.device("cuda", 0))
    with pytest.raises(ValueError, match="mixed-size batch needs a program that takes any size"):
        Engine._io_mixed(teacher, canvas, OP_SIZES)
    student = types.SimpleNamespace(program=AttentionStudent(None, "cpu", inplanes=48).compile_program(), device=torch.device("cuda", 0))
    with pytest.raises(ValueError, match="at least 32"):
        Engine._io_mixed(student, canvas, [(31, 47), (47, 33), (64, 32)])
    with pytest.raises(RuntimeError, match="executor lives on"):
        Engine._io_mixed(student, canvas, OP_SIZES)
    student.program.has_aux = True
    with pytest.raises(ValueError, match="second input"):
        Engine._io_mixed(student, canvas, OP_SIZES)


def test_student_pipeline_keeps_its_refusals_and_does_not_stream_mixed_batches():
    from rtpe.engine import StudentPipeline
    from test_student_pipeline_host import _parser

    class NoForward(torch.nn.Module):
        def forward(self, x, alt=None):
            raise AssertionError("GPU work")

        def forward_mixed(self, canvas, sizes):
            raise AssertionError("GPU work")
    pipe = StudentPipeline.__new__(StudentPipeline)         # (the constructor moves the model to a GPU)
    pipe.model, pipe.parser = NoForward(), _parser()
    pipe.flip_test, pipe.scale_factors, pipe.ags = False, None, False
    pipe.device = torch.device("cpu")
    x = torch.zeros((2, 3, 96, 128))
    with pytest.raises(ValueError, match="one decode size"):            # as before
        pipe(x, out_hw=[(96, 128), (90, 120)])
    ims = _images(OP_SIZES)
    from rtpe.students import pack_mixed
    for batch in (ims, tuple(ims), pack_mixed(ims)):
        with pytest.raises(ValueError, match="call_mixed"):
            pipe(batch)
        with pytest.raises(ValueError, match="call_mixed"):           # the first thing stream() does with a batch
            pipe._decode_hw(None, batch)
    assert not pipe._is_mixed(x) and not pipe._is_mixed((x, x)) and not pipe._is_mixed((x, None)) and not pipe._is_mixed([x, x, x])
    with pytest.raises(ValueError, match="at least 32"):
        pipe.call_mixed([torch.zeros(3, 31, 40)])
    with pytest.raises(ValueError, match="2 image ids for 3 images"):
        pipe.call_mixed(ims, image_ids=[1, 2])
    with pytest.raises(AssertionError, match="GPU work"):
        pipe.call_mixed(ims)
    pipe.model = torch.nn.Identity()
    with pytest.raises(ValueError, match="no forward_mixed"):
        pipe.call_mixed(ims)


# --------------------------------------------------------------------------- #
# the premise: zero padding is not an answer
# --------------------------------------------------------------------------- #
def test_zero_padding_to_a_canvas_changes_det_inside_the_image(golden_dir):
    """the s100 student on the 33 x 47 fixture image (seed 101, image 0) alone and zero-padded into 33 x 64, 64 x 47 and
    40 x 52 canvases: inside the image's own 9 x 12 region ``det`` moves by far more than ``S.within`` allows (measured
    0.26, 0.34 and 0.49 at a range of 0.70) - behind the first BatchNorm the padding is no longer zero.  So an unmasked
    kernel cannot pass the GPU tests of the mixed forward."""
    sd = S.student_sd(golden_dir, "s100")
    x = synth.make_images(2, 33, 47, seed=101)[:1]
    att0, det0 = [t.numpy() for t in student_ref.student_forward(sd, x, half_stem=True)]
    assert det0.shape == (1, 18, 9, 12)
    bound = 1e-3 * max(1.0, float(np.abs(det0).max()))
    for Hc, Wc in ((33, 64), (64, 47), (40, 52)):
        canvas = torch.zeros(1, 3, Hc, Wc)
        canvas[:, :, :33, :47] = x
        att, det = [t.numpy() for t in student_ref.student_forward(sd, canvas, half_stem=True)]
        diff = np.abs(det[:, :, :9, :12] - det0)
        print("zero-padded into %d x %d: det differs by %.3f inside the image (range %.2f), %.0f %% of the elements by more "
              "than 1e-3; att by %.1e" % (Hc, Wc, diff.max(), np.ptp(det0), 100 * (diff > 1e-3).mean(),
                                          np.abs(att[:, :, :9, :12] - att0).max()))
        assert diff.max() > 100 * bound and (diff > bound).mean() > 0.5
        with pytest.raises(AssertionError):
            S.within((att[:, :, :9, :12], det[:, :, :9, :12]), (att0, det0), "padded vs alone")
