"""CPU tests of the students at input sizes that are not multiples of 32: the extent rule, the nearest-to-size index rule of
the fuse op, the fixture of the reference's outputs at such sizes (tests/golden/student_sizes.npz, written by
tools/gen_golden_student_sizes.py) against the oracle, the ABI of the new entries, and the refusals that come before any
GPU work.  The case tables of tests/test_student_sizes_gpu.py live here."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import student_ref, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(min(16, torch.get_num_threads()))

# the fixture's cases (tools/gen_golden_student_sizes.py): name, N, H, W, seed of the images [, seed of alt, att_divisor]
S100_CASES = (("33x47", 2, 33, 47, 101), ("100x140", 1, 100, 140, 102), ("427x640", 1, 427, 640, 103))
STEPS_CASES = (("33x47", 1, 33, 47, 111, 112, None), ("100x140", 1, 100, 140, 113, 114, 20.0))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


def steps_alt(n, h, w, seed):
    rgb = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))
    lab = student_ref.rgb2lab(rgb.permute(0, 2, 3, 1).numpy()).astype(np.float32)
    return torch.from_numpy(lab).permute(0, 3, 1, 2).contiguous()


def student_sd(golden_dir, which):
    """the seeded state dicts of student.npz / student_steps.npz"""
    name, seed = {"s100": ("student_shapes.json", 3), "steps": ("student_steps_shapes.json", 4)}[which]
    shapes = json.load(open(os.path.join(golden_dir, name)))["shapes"]
    return synth.make_state_dict({k: tuple(v) for k, v in shapes.items()}, seed, "W1")


def within(got, want, what):
    """the bound of the students' GPU tests (BASELINE's heat-map tolerance): |att - ref| <= 1e-3 and
    |det - ref| <= 1e-3 * max(1, |ref det| max); prints the figures first"""
    (ga, gd), (wa, wd) = got, want
    assert ga.shape == wa.shape and gd.shape == wd.shape, (what, ga.shape, wa.shape, gd.shape, wd.shape)
    ea, ed, rng = float(np.abs(ga - wa).max()), float(np.abs(gd - wd).max()), max(1.0, float(np.abs(wd).max()))
    print("%s: att %.3e det %.3e (|det| max %.3f)" % (what, ea, ed, float(np.abs(wd).max())))
    assert np.isfinite(ga).all() and np.isfinite(gd).all(), what
    assert ea <= 1e-3 and ed <= 1e-3 * rng, (what, ea, ed)


def fixture_case(g, prefix, name):
    """(att, det) of a fully stored case, or None for the sampled one"""
    key = "%s_%s_att" % (prefix, name)
    return (g[key], g["%s_%s_det" % (prefix, name)]) if key in g.files else None


def sampled_within(g, prefix, name, att, det, what):
    """the 427 x 640 case: every 4th row and column with the bound of ``within``, and the sums within what that bound allows
    for all elements together"""
    sa, sd_ = g["%s_%s_att_s4" % (prefix, name)], g["%s_%s_det_s4" % (prefix, name)]
    within((att[:, :, ::4, ::4], det[:, :, ::4, ::4]), (sa, sd_), what)
    rng = max(1.0, float(np.abs(sd_).max()))
    for key, t, tol in (("att", att, 1e-3), ("det", det, 1e-3 * rng)):
        for kind, v in (("sum", t.astype(np.float64).sum()), ("abs", np.abs(t.astype(np.float64)).sum())):
            want = float(g["%s_%s_%s_%s" % (prefix, name, key, kind)])
            print("%s: %s %s %.6f against %.6f" % (what, key, kind, v, want))
            assert abs(v - want) <= tol * t.size, (what, key, kind, v, want)


# --------------------------------------------------------------------------- #
# extent rule
# --------------------------------------------------------------------------- #
def test_extent_gives_the_reference_shapes_and_the_old_ones_for_multiples_of_32(built):
    from rtpe._native import extent, ragged
    # the reference's students on the CPU (ISSUE: 427 x 640 -> 107 x 160, 100 x 140 -> 25 x 35, 33 x 47 -> 9 x 12)
    for (h, w), (h4, w4) in (((427, 640), (107, 160)), ((100, 140), (25, 35)), ((33, 47), (9, 12)), ((640, 480), (160, 120))):
        assert (extent(h, 2), extent(w, 2)) == (h4, w4)
    # every map is the ceil chain: d stride-2 convs with padding k // 2 / AvgPool2d(3, 2, 1)
    for n in list(range(32, 200)) + [427, 640, 719, 720, 1081]:
        x = torch.zeros(1, 1, n, 1)
        m = n
        for d in range(1, 6):
            x = F.avg_pool2d(x, 3, 2, 1, count_include_pad=False)
            m = F.conv2d(torch.zeros(1, 1, m, 1), torch.zeros(1, 1, 5, 5), None, 2, 2).shape[2]
            assert extent(n, d) == x.shape[2] == m == -(-n // (1 << d)), (n, d)
    for n in range(32, 2049, 32):
        assert not ragged(n, n) and ragged(n + 1, n) and ragged(n, n - 1)
        for d in range(0, 6):
            assert extent(n, d) == n >> d == -(-n // (1 << d))
        assert extent(n, 6) == n >> 6                     # (32 at ds = 6: a tensor without pixels, as ever)
    assert extent(32, 6) == 0 and extent(33, 6) == 1
    lib = built.lib()
    for n in (32, 33, 47, 64, 100, 427, 640, 2048):
        for d in range(0, 8):
            assert lib.rtpe_extent(n, d) == extent(n, d), (n, d)
    assert lib.rtpe_extent(0, 2) == 0 and lib.rtpe_extent(33, -1) == 0


def test_anysize_symbols_are_declared_in_their_header_and_resolve(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtpe_hip_anysize.h")).read(), flags=re.S)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtpe_hip.h")).read(), flags=re.S)
    assert len(re.findall(r'#include "rtpe_hip_anysize.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(built.EXPORTS_ANYSIZE) == {"rtpe_extent", "rtpe_nearest_src", "rtpe_hrnet_set_any_size",
                                                      "rtpe_hrnet_get_any_size"}
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR,
             built.EXPORTS_RECORDS, built.EXPORTS_TAGMEAN, built.EXPORTS_NOPROJ)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2, 6, 5]          # no change to the existing tables
    for table in older:
        assert not declared & set(table)
    lib = built.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == built._SIGS_ANYSIZE[name][1]
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4
    assert lib.rtpe_hrnet_set_any_size(None, 1) != 0 and b"set_any_size" in lib.rtpe_last_error_string()


# --------------------------------------------------------------------------- #
# nearest-to-size index rule
# --------------------------------------------------------------------------- #
def _torch_nearest_index(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return F.interpolate(src, size=(n_out, 1), mode="nearest").flatten().long().numpy()


def test_nearest_restatement_equals_interpolate_for_every_pair_of_the_ceil_chain(built):
    """stem sides 8 .. 512 (inputs 29 .. 2048): the detection head's 2x pair and the attention head's 4x pair"""
    from rtpe._native import nearest_src
    lib = built.lib()
    differs_from_shift = {1: 0, 2: 0}
    for out in range(8, 513):
        for up in (1, 2):
            n_in = -(-out // (1 << up))
            want = _torch_nearest_index(n_in, out)
            got = nearest_src(np.arange(out), n_in, out)
            assert np.array_equal(got, want), (n_in, out)
            shift = np.minimum(np.arange(out) >> up, n_in - 1)
            differs_from_shift[up] += int(not np.array_equal(shift, want))
            if out % 37 == 0 or out < 16:
                assert [lib.rtpe_nearest_src(i, n_in, out) for i in range(out)] == want.tolist(), (n_in, out)
    # the shift `dst >> up` is the rule only where out == in << up: it is wrong for 4x pairs (3 -> 9: 0 0 0 1 1 1 2 2 2,
    # not 0 0 0 0 1 1 1 1 2), never for the 2x pairs of the ceil chain
    assert differs_from_shift[1] == 0 and differs_from_shift[2] > 100
    assert nearest_src(np.arange(9), 3, 9).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert lib.rtpe_nearest_src(9, 3, 9) == -1 and lib.rtpe_nearest_src(-1, 3, 9) == -1 and lib.rtpe_nearest_src(0, 0, 9) == -1


# --------------------------------------------------------------------------- #
# the fixture against the oracle
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def sizes_npz(golden_dir):
    path = os.path.join(golden_dir, "student_sizes.npz")
    assert os.path.getsize(path) < 1 << 20
    return np.load(path)


def test_oracle_matches_the_reference_fixture_at_ragged_sizes(golden_dir, sizes_npz):
    g = sizes_npz
    sd = student_sd(golden_dir, "s100")
    for name, n, h, w, seed in S100_CASES:
        oa, od = [t.numpy() for t in student_ref.student_forward(sd, synth.make_images(n, h, w, seed=seed), half_stem=True)]
        assert oa.shape == (n, 1, -(-h // 4), -(-w // 4)) and od.shape == (n, 18, -(-h // 4), -(-w // 4))
        full = fixture_case(g, "s100", name)
        if full is None:
            sampled_within(g, "s100", name, oa, od, "oracle vs reference student100 " + name)
        else:
            within((oa, od), full, "oracle vs reference student100 " + name)
    sd = student_sd(golden_dir, "steps")
    for name, n, h, w, seed, alt_seed, div in STEPS_CASES:
        x, alt = synth.make_images(n, h, w, seed=seed), steps_alt(n, h, w, alt_seed)
        oa, od = [t.numpy() for t in student_ref.student_steps_forward(sd, x, alt, div, half_stem=True)]
        within((oa, od), fixture_case(g, "steps", name), "oracle vs reference steps48 " + name)
    # what the generator measured on its machine
    assert g["oracle_vs_reference_maxdiff"].shape == (5, 2) and float(g["oracle_vs_reference_maxdiff"].max()) <= 1e-3
    assert float(g["bundled_oracle_vs_reference_maxdiff"].max()) <= 1e-3


# --------------------------------------------------------------------------- #
# the property and the refusals before any GPU work
# --------------------------------------------------------------------------- #
class _CudaTensorStandIn:
    """what Engine._io looks at before it allocates anything: a float32 (N, 3, H, W) tensor on cuda:0"""

    def __init__(self, n, h, w):
        self.shape, self.dtype, self.is_cuda, self.device = (n, 3, h, w), torch.float32, True, torch.device("cuda", 0)

    def dim(self):
        return 4

    def contiguous(self):
        return self


def _io(program, n, h, w):
    from rtpe.third_party.pose_higher_hrnet import Engine
    eng = types.SimpleNamespace(program=program, device=torch.device("cuda", 0))
    return Engine._io(eng, _CudaTensorStandIn(n, h, w), torch.float32)


def test_students_have_the_property_the_teacher_does_not_and_refusals_come_first():
    from rtpe.students import AttentionStudent, AttentionStudentSteps
    from rtpe.third_party.pose_higher_hrnet import PoseHigherResolutionNet, ProgramBuilder
    assert ProgramBuilder().any_size is False and ProgramBuilder(any_size=True).finish().any_size is True
    students = [AttentionStudent(None, "cpu", inplanes=48).compile_program(),
                AttentionStudent(None, "cpu", inplanes=64, half_precision=False).compile_program(),
                AttentionStudentSteps(None, "cpu", inplanes=48).compile_program()]
    assert all(p.any_size is True for p in students)
    teacher = PoseHigherResolutionNet().eval().compile_program()
    assert teacher.any_size is False
    with pytest.raises(ValueError, match="multiples of 32.*fused by factor-2 resampling"):
        _io(teacher, 1, 100, 140)
    with pytest.raises(ValueError, match="multiples of 32"):
        _io(teacher, 1, 128, 100)
    for p in students + [teacher]:
        for hw in ((31, 47), (47, 31), (16, 16), (0, 64)):
            with pytest.raises(ValueError, match="at least 32"):
                _io(p, 1, *hw)
    # ragged shapes never ask for tuning
    from rtpe.third_party.pose_higher_hrnet import Engine
    eng = types.SimpleNamespace(_tuned=set())
    assert Engine._wants_tuning(eng, 1, 320, 320) is (os.environ.get("RTPE_AUTOTUNE", "1") != "0")
    assert Engine._wants_tuning(eng, 1, 100, 140) is False and Engine._wants_tuning(eng, 1, 320, 427) is False
