"""CPU tests of the device-resident keypoint records: the ABI of the two new entries (their own header, the binding's
table), the refusals of ``rtpe_pack_records`` before any launch, ``transforms.final_preds_matrix`` against
``get_final_preds``, and the pure-numpy restatement of the record - the function the GPU kernel test compares against -
pinned on ``engine.pack_records`` + ``get_final_preds`` first."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J, P = 17, 30
COUNTS = [0, 3, 31, 1, 30]          # empty, short, truncated, single, exactly full


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


# ---- the restatement and the seeded inputs shared with tests/test_records_gpu.py ------------------------------------
def records_restated(rows, scores, counts, ids, xform=None, max_people=P):
    """the record tensor in plain numpy: rows (cap, J, C >= 4) f32, scores (cap) f32, counts / ids (N) ints, xform None
    or (N, 6) f64.  Rows and scores at and beyond sum(counts) are not read."""
    rows, scores = np.asarray(rows, np.float32), np.asarray(scores, np.float32)
    n_img, nj = len(counts), rows.shape[1]
    rec = np.zeros((n_img, 2 + max_people + max_people * nj * 4), np.float32)
    o = 0
    for i in range(n_img):
        n = min(int(counts[i]), max_people)
        rec[i, 0], rec[i, 1] = np.float32(ids[i]), np.float32(n)
        rec[i, 2:2 + n] = scores[o:o + n]
        kp = rows[o:o + n, :, :4].copy()
        if xform is not None and n:
            t = np.asarray(xform[i], np.float64)
            x, y = kp[..., 0].astype(np.float64), kp[..., 1].astype(np.float64)
            kp[..., 0] = ((t[0] * x + t[1] * y) + t[2]).astype(np.float32)
            kp[..., 1] = ((t[3] * x + t[4] * y) + t[5]).astype(np.float32)
        rec[i, 2 + max_people:2 + max_people + n * nj * 4] = kp.reshape(-1)
        o += int(counts[i])
    return rec


def kernel_inputs(C, seed=5, cap=80):
    """seeded inputs of the kernel test: ``rows (cap, J, C), scores (cap), counts, ids, xform (N, 6)`` with NaN in the
    rows and scores beyond the total; coordinates U(0, 640), matrix entries U(-2, 2), offsets x 300"""
    rng = np.random.default_rng(seed)
    total = sum(COUNTS)
    assert cap > total
    rows = np.full((cap, J, C), np.nan, np.float32)
    rows[:total] = rng.normal(0, 2, (total, J, C)).astype(np.float32)
    rows[:total, :, 0:2] = rng.uniform(0, 640, (total, J, 2)).astype(np.float32)
    rows[:total, :, 2] = rng.random((total, J)).astype(np.float32)
    rows[:total:3, 5, 2] = 0                                 # joints without a detection are transformed too
    scores = np.full((cap,), np.nan, np.float32)
    scores[:total] = rng.random(total).astype(np.float32)
    xform = rng.uniform(-2, 2, (len(COUNTS), 6))
    xform[:, [2, 5]] *= 300
    ids = np.array([7, 1 << 24, 0, 581929, 42], np.int32)
    return rows, scores, np.array(COUNTS, np.int32), ids, xform


def _lists(rows, scores, counts):
    """the per-image ``(people, scores)`` lists that ``lowres_finish`` returns for these rows"""
    out, o = [], 0
    for c in counts:
        c = int(c)
        out.append((rows[o:o + c].copy() if c else np.array([], np.float32), [np.float32(v) for v in scores[o:o + c]]))
        o += c
    return out


def _as_transform_preds(people, t):
    """``transforms.transform_preds`` with the matrix given: ``affine_transform`` of every row, assigned in place"""
    from rtpe.third_party.transforms import affine_transform
    out = people.copy()
    t = np.asarray(t, np.float64).reshape(2, 3)
    for p in range(people.shape[0]):            # (as get_final_preds: every person, every joint)
        for j in range(people.shape[1]):
            out[p, j, 0:2] = affine_transform(people[p, j, 0:2], t)
    return out


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_records_symbols_are_declared_and_resolve(built):
    from rtpe import engine
    main = _declared("rtpe_hip.h")
    assert len(re.findall(r'#include "rtpe_hip_records.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_records.h")))
    assert declared == {"rtpe_records_floats", "rtpe_pack_records"} == set(built.EXPORTS_RECORDS)
    for older in (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR):
        assert not declared & set(older)
    assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", main))
    lib = built.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == built._SIGS_RECORDS[name][1], name
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4
    nf = ctypes.c_size_t()
    assert lib.rtpe_records_floats(17, 30, ctypes.byref(nf)) == 0
    assert nf.value == engine.RECORD_FLOATS == 2072
    assert lib.rtpe_records_floats(3, 5, ctypes.byref(nf)) == 0 and nf.value == 2 + 5 + 5 * 3 * 4
    for bad in ((0, 30, ctypes.byref(nf)), (17, 0, ctypes.byref(nf)), (17, 30, None)):
        assert lib.rtpe_records_floats(*bad) < 0


def test_pack_records_refuses_bad_arguments_before_any_launch(built):
    """negative codes and a message; nothing is launched: the pointers are never read (there is no GPU here)"""
    L = built.lib()
    fake = ctypes.c_void_p(0x1000)
    good = dict(rows=fake, C=4, scores=fake, counts=fake, ids=fake, xform=None, N=5, J=17, cap=80, P=30, rec=fake,
                rec_bytes=5 * 2072 * 4, stream=None)

    def call(**kw):
        return L.rtpe_pack_records(*dict(good, **kw).values())
    for kw in (dict(rows=None), dict(scores=None), dict(counts=None), dict(ids=None), dict(rec=None),
               dict(N=0), dict(N=-1), dict(J=0), dict(J=-17), dict(cap=0), dict(cap=-80), dict(P=0), dict(P=-30),
               dict(C=3), dict(C=0), dict(rec_bytes=5 * 2072 * 4 - 1), dict(rec_bytes=0),
               dict(xform=fake, rec_bytes=4 * 2072 * 4)):
        assert call(**kw) < 0, kw
        assert b"pack_records" in L.rtpe_last_error_string(), kw
    assert call(C=3) < 0 and b"at least 4" in L.rtpe_last_error_string()
    assert call(rec_bytes=8) < 0 and b"rec of 8 bytes" in L.rtpe_last_error_string()


# ---- final_preds_matrix --------------------------------------------------------------------------------------------------
class _Img:
    def __init__(self, h, w):
        self.shape = (h, w, 3)


@pytest.mark.parametrize("hw,scales,want_size", [((480, 640), (1,), (896, 640)), ((555, 640), (1,), (768, 640)),
                                                 ((480, 640), (2, 1, 0.5), None)])
def test_final_preds_matrix_reproduces_get_final_preds(hw, scales, want_size):
    """applied as ``affine_transform`` does, the 6 values give the bits of ``get_final_preds`` - at the two bundled
    geometries (640x480 -> 896x640, 640x555 -> 768x640) and at a multi-scale base size with the centre / scale of the
    smallest scale's warp, as the batched drivers use it"""
    from rtpe.third_party import transforms
    lo = min(scales)
    base, _, _ = transforms.get_multi_scale_size(_Img(*hw), 640, 1.0, lo)
    _, center, scale = transforms.get_multi_scale_size(_Img(*hw), 640, lo, lo)
    if want_size is not None:
        assert tuple(base) == want_size
    m = transforms.final_preds_matrix(center, scale, list(base))
    assert m.shape == (6,) and m.dtype == np.float64
    assert np.array_equal(m.reshape(2, 3), transforms.get_affine_transform(center, scale, 0, list(base), inv=1))
    rng = np.random.default_rng(3)
    people = rng.normal(0, 2, (7, J, 5)).astype(np.float32)
    people[..., 0] = rng.uniform(0, base[0], (7, J)).astype(np.float32)
    people[..., 1] = rng.uniform(0, base[1], (7, J)).astype(np.float32)
    want = np.stack(transforms.get_final_preds([people], center, scale, list(base)))
    got = _as_transform_preds(people, m)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got[..., :2], people[..., :2]) and np.array_equal(got[..., 2:], people[..., 2:])
    # ... and so does the restatement's arithmetic
    rec = records_restated(people, np.zeros(7, np.float32), [7], [1], m[None])
    assert np.array_equal(rec[0, 2 + P:2 + P + 7 * J * 4].reshape(7, J, 4), want[..., :4])


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 5])
def test_restatement_equals_pack_records(C):
    """on seeded rows: without a transform, with the matrices of ``get_final_preds`` (centre / scale), and with
    arbitrary seeded matrices applied as ``transform_preds`` applies ``affine_transform``"""
    from rtpe import engine
    from rtpe.third_party import transforms
    rows, scores, counts, ids, xform = kernel_inputs(C)
    total = int(counts.sum())
    lists = _lists(rows, scores, counts)
    want = engine.pack_records(ids.tolist(), lists, "cpu").numpy()
    got = records_restated(rows, scores, counts, ids)
    assert got.shape == (5, engine.RECORD_FLOATS) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert want[:, 1].tolist() == [0, 3, 30, 1, 30] and want[:, 0].tolist() == [7, 1 << 24, 0, 581929, 42]
    assert not np.isnan(want).any()

    geo = [transforms.get_multi_scale_size(_Img(h, w), 640, 1.0, 1) for h, w in
           ((480, 640), (555, 640), (640, 480), (427, 640), (500, 375))]
    final = [(np.stack(transforms.get_final_preds([p], c, s, list(size))) if len(p) else p, sc)
             for (p, sc), (size, c, s) in zip(lists, geo)]
    mats = np.stack([transforms.final_preds_matrix(c, s, list(size)) for size, c, s in geo])
    want = engine.pack_records(ids.tolist(), final, "cpu").numpy()
    got = records_restated(rows, scores, counts, ids, mats)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

    moved = [(_as_transform_preds(p, t) if len(p) else p, sc) for (p, sc), t in zip(lists, xform)]
    want = engine.pack_records(ids.tolist(), moved, "cpu").numpy()
    got = records_restated(rows, scores, counts, ids, xform)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(rows[total:]).all() and np.isnan(scores[total:]).all()


def test_kernel_inputs_tell_float32_from_float64():
    """the seeded inputs of the kernel test: an evaluation of the affine in float32 differs from the float64 one"""
    rows, scores, counts, ids, xform = kernel_inputs(4)
    total = int(counts.sum())
    pimg = np.repeat(np.arange(len(counts)), counts)
    t = xform[pimg][:, None, :]                                # (total, 1, 6)
    x, y = rows[:total, :, 0], rows[:total, :, 1]
    t32 = t.astype(np.float32)
    f32 = np.stack(((t32[..., 0] * x + t32[..., 1] * y) + t32[..., 2], (t32[..., 3] * x + t32[..., 4] * y) + t32[..., 5]))
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    f64 = np.stack(((t[..., 0] * x64 + t[..., 1] * y64) + t[..., 2],
                    (t[..., 3] * x64 + t[..., 4] * y64) + t[..., 5])).astype(np.float32)
    assert f32.dtype == np.float32
    differ = int((f32 != f64).sum())
    print("float32 against float64 affine: %d of %d elements differ" % (differ, f64.size))
    assert differ >= 1


# ---- refusals of the parser, the pipeline and the drivers before any GPU work -------------------------------------------
def _parser(match_on="device", joints=17, people=30):
    from rtpe.third_party.group import HeatmapParser
    return HeatmapParser(joints, people, 0.1, 1.0, True, False, match_on=match_on)


def test_check_records_refusals_and_round_trip(built):
    p = _parser()
    assert p.check_records(3, None) is None
    ids, xf = p.check_records(3, ([5, 0, 1 << 24], None))
    assert ids.dtype == np.int32 and ids.tolist() == [5, 0, 1 << 24] and xf is None
    ids, xf = p.check_records(2, (np.array([1, 2]), [[1, 0, 0, 0, 1, 0]] * 2))
    assert xf.dtype == np.float64 and xf.shape == (2, 6)
    ids2, xf2 = p.check_records(2, (ids, xf))                   # what it returns is accepted again
    assert np.array_equal(ids2, ids) and np.array_equal(xf2, xf)
    for n, rec, word in ((3, ([1, 2, (1 << 24) + 1], None), "2\\*\\*24"), (3, ([1, -2, 3], None), "2\\*\\*24"),
                         (3, ([1, 2], None), "2 image ids for 3"), (2, ([1, 2], np.zeros((2, 5))), "xform"),
                         (2, ([1, 2], np.zeros((3, 6))), "xform"), (2, ([1, 2], np.zeros(12)), "xform"),
                         (2, ([1.5, 2], None), "integers"), (2, [1, 2, 3], "image_ids, xform")):
        with pytest.raises(ValueError, match=word):
            p.check_records(n, rec)
    with pytest.raises(ValueError, match="match_on='device'"):
        _parser("host").check_records(2, ([1, 2], None))
    with pytest.raises(ValueError, match="17 joints and 30 people"):
        _parser(joints=18).check_records(2, ([1, 2], None))
    with pytest.raises(ValueError, match="17 joints and 30 people"):
        _parser(people=20).check_records(2, ([1, 2], None))
    # lowres_match refuses on the state's N before touching anything else of it
    with pytest.raises(ValueError, match="3 image ids for 2"):
        p.lowres_match({"N": 2}, records=([1, 2, 3], None))
    with pytest.raises(ValueError, match="match_on='device'"):
        _parser("host").lowres_match({"N": 2}, records=([1, 2], None))


def test_drivers_refuse_image_ids_without_device_grouping(built):
    from rtpe import inference
    imgs = [np.zeros((120, 160, 3), np.uint8)] * 2
    for fn in (inference.plain_inference, inference.flip_test_inference, inference.multi_scale_batch_inference):
        with pytest.raises(ValueError, match="match_on='device'"):
            fn(None, _parser("host"), imgs, input_size=128, image_ids=[1, 2])
        with pytest.raises(ValueError, match="match_on='device'"):
            fn(None, _parser("device"), imgs, input_size=128, image_ids=[1, 2], match_on="host")
        with pytest.raises(ValueError, match="1 image ids for 2"):
            fn(None, _parser("device"), imgs, input_size=128, image_ids=[1])
        with pytest.raises(ValueError, match="2\\*\\*24"):
            fn(None, _parser("host"), imgs, input_size=128, image_ids=[1, (1 << 24) + 1], match_on="device")


def test_gather_takes_a_record_tensor_as_it_is():
    from rtpe import engine
    pipe = engine.TeacherPipeline.__new__(engine.TeacherPipeline)      # gather reads self.device only
    pipe.device = torch.device("cpu")
    rec = torch.arange(2 * engine.RECORD_FLOATS, dtype=torch.float32).reshape(2, -1)
    assert pipe.gather(None, rec) is rec
    with pytest.raises(ValueError, match="image_ids=None"):
        pipe.gather([1, 2], rec)
    with pytest.raises(ValueError, match="record tensor"):
        pipe.gather(None, rec[:, :100])
