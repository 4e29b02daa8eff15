"""The device-resident keypoint records (csrc/records.hip, HeatmapParser.lowres_match(records=...), the pipelines'
``image_ids`` / ``records``, the drivers' ``image_ids``) against the host path in the same process:
``engine.pack_records`` of the list results, after ``transforms.get_final_preds`` where a transform applies.  Whole
tensors, ``torch.equal`` / ``np.array_equal``."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import synth
from test_match_device_gpu import _ags_outputs, _blob_outputs, _parser, _scale_outputs
from test_multiscale_decode_gpu import H, W, _small_batches, _small_pipe
from test_records_host import COUNTS, J, P, _as_transform_preds, kernel_inputs, records_restated
from test_student_pipeline_gpu import STREAM_HW, _StandIn, stream_case  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMBOS = [(True, True), (False, False)]


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


@pytest.fixture(scope="module")
def teacher(nat, w48_shapes):
    from rtpe.helpers import build_hrnet_w48_teacher
    sd = synth.make_state_dict(w48_shapes, 0, "W0")
    return build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(DEV)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _xform(n, seed=77):
    """seeded float64 matrices: entries U(-2, 2), offsets x 300"""
    t = np.random.default_rng(seed).uniform(-2, 2, (n, 6))
    t[:, [2, 5]] *= 300
    return t


def _n(people):
    return len(people) if getattr(people, "ndim", 0) == 3 else 0


def _host_records(ids, results, xform=None, min_each=None):
    """``pack_records`` of a list result, the rows moved as ``transform_preds`` moves them when ``xform`` is given;
    ``min_each``: every image must hold that many people"""
    from rtpe import engine
    if min_each is not None:
        assert all(_n(p) >= min_each for p, _ in results), [_n(p) for p, _ in results]
    if xform is not None:
        results = [(_as_transform_preds(p, t) if _n(p) else p, s) for (p, s), t in zip(results, xform)]
    return engine.pack_records(list(ids), results, "cpu")


def _turns(parser):
    """where the parser's rings of 4 pinned host buffers stand (``HeatmapParser._pinned``).  A records batch is never
    waited for by the host, so it may take nothing from a ring: the turns must not advance while one is decoded.
    This holds the reuse rule without depending on how far the host happens to run ahead of the GPU."""
    return dict(parser.__dict__.get("_pin_turn", {}))


def _equal(rec, want):
    assert rec.is_cuda and rec.dtype == torch.float32 and tuple(rec.shape) == tuple(want.shape)
    got = rec.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))       # the bits (signed zeros)
    assert not torch.isnan(got).any()


# ---- the kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("with_xform", [False, True])
@pytest.mark.parametrize("C", [4, 5])
def test_pack_records_kernel_equals_the_restatement(nat, C, with_xform, pinned):
    """counts [0, 3, 31, 1, 30] (empty, short, truncated, single, exactly full), cap above the total with NaN beyond
    it, rec pre-filled with NaN between NaN guard bands: every float written, nothing outside.  Sources in device
    memory and in pinned memory read in place; a second run with the records 12 bytes off a 16-byte boundary takes the
    kernel's 4-byte stores."""
    L = nat.lib()
    rows, scores, counts, ids, xform = kernel_inputs(C)
    cap, nf = rows.shape[0], 2 + P + P * J * 4
    want = records_restated(rows, scores, counts, ids, xform if with_xform else None)

    def place(a):
        t = torch.from_numpy(a)
        return t.pin_memory() if pinned else t.to(DEV)
    d_rows, d_scores, d_counts, d_ids = place(rows), place(scores), place(counts), place(ids)
    d_xf = place(xform) if with_xform else None
    for guard in (64, 67):                                   # floats in front: 16-byte aligned records, then not
        buf = torch.full((guard + 5 * nf + 64,), float("nan"), dtype=torch.float32, device=DEV)
        rec = buf[guard:guard + 5 * nf]
        assert (rec.data_ptr() % 16 == 0) == (guard == 64)
        nat.check(L.rtpe_pack_records(_ptr(d_rows), C, _ptr(d_scores), _ptr(d_counts), _ptr(d_ids),
                                      _ptr(d_xf) if with_xform else None, 5, J, cap, P, _ptr(rec), rec.numel() * 4,
                                      nat.stream_ptr(torch.device(DEV))))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.isnan(got[:guard]).all() and np.isnan(got[guard + 5 * nf:]).all()
        body = got[guard:guard + 5 * nf].reshape(5, nf)
        assert not np.isnan(body).any()
        assert np.array_equal(body.view(np.uint32), want.view(np.uint32))
    assert want[:, 1].tolist() == [min(c, P) for c in COUNTS]


# ---- every protocol ---------------------------------------------------------------------------------------------------
def _both(parse, n, adjust, refine, with_xform, min_each=1):
    """``parse(parser, **kw)`` with the list path and with records, both on the device matcher"""
    ids = [1000 + 3 * i for i in range(n)]
    xform = _xform(n) if with_xform else None
    lists = parse(_parser(match_on="device"), adjust=adjust, refine=refine)
    p = _parser(match_on="device")
    rec = parse(p, adjust=adjust, refine=refine, records=(ids, xform))
    assert _turns(p) == {}                                      # nothing of a records batch comes from a ring
    _equal(rec, _host_records(ids, lists, xform, min_each))
    return lists


@pytest.mark.parametrize("with_xform", [False, True])
@pytest.mark.parametrize("adjust,refine", COMBOS)
@pytest.mark.parametrize("sizes", [False, True])
def test_parse_lowres_records(nat, adjust, refine, with_xform, sizes):
    Pm, R, _, _ = _blob_outputs(4, 192, 256, seed=21)
    hw = [(192, 256), (180, 250), (200, 256), (192, 230)] if sizes else (192, 256)
    _both(lambda p, **kw: p.parse_lowres(R, Pm[:, J:], hw, **kw), 4, adjust, refine, with_xform)


@pytest.mark.parametrize("with_xform", [False, True])
@pytest.mark.parametrize("adjust,refine", COMBOS)
def test_parse_lowres_shared_records(nat, adjust, refine, with_xform):
    Pm, R, _, _ = _blob_outputs(4, 192, 256, seed=21)
    tag = Pm[:, J:].amax(1, keepdim=True).contiguous()              # ONE tag map per image (at half the heat maps' size)
    _both(lambda p, **kw: p.parse_lowres_shared(R, tag, (192, 256), **kw), 4, adjust, refine, with_xform)


@pytest.mark.parametrize("with_xform", [False, True])
@pytest.mark.parametrize("adjust,refine", COMBOS)
def test_parse_flip_records(nat, adjust, refine, with_xform):
    outs = _blob_outputs(3, 192, 320, seed=33)
    lists = _both(lambda p, **kw: p.parse_flip(*outs, **kw), 3, adjust, refine, with_xform)
    assert lists[0][0].shape[1:] == (J, 5)                          # the mirror image's tag is dropped


@pytest.mark.parametrize("with_xform", [False, True])
@pytest.mark.parametrize("adjust,refine", COMBOS)
@pytest.mark.parametrize("ags", [False, True])
@pytest.mark.parametrize("flip", [True, False])
def test_parse_multi_scale_records(nat, flip, ags, adjust, refine, with_xform):
    order = (2, 1, 0.5)
    made = _ags_outputs(3, order, seed=31) if ags else _scale_outputs(3, order, seed=50)
    outs = [o if flip else o[:2] for o in made]
    _both(lambda p, **kw: p.parse_multi_scale(outs, (H, W), order, flip, ags=ags, **kw), 3, adjust, refine, with_xform)


def test_records_of_images_without_people(nat):
    """the batch of test_images_without_people (images 0, 2 and 4 empty) and an all-zero batch: n = 0 exactly there"""
    Pm, R, Pf, Rf = _blob_outputs(5, 192, 256, seed=61)
    for t in (R, Rf):
        t[0] = 0
        t[2] = 0
        t[4] = 0
    for adjust, refine in COMBOS:
        for xf in (False, True):
            lists = _both(lambda p, **kw: p.parse_lowres(R, Pm[:, J:], (192, 256), **kw), 5, adjust, refine, xf, 0)
            assert [_n(p) > 0 for p, _ in lists] == [False, True, False, True, False]
            _both(lambda p, **kw: p.parse_flip(Pm, R, Pf, Rf, **kw), 5, adjust, refine, xf, 0)
    dev = _parser(match_on="device")
    rec = dev.parse_lowres(R, Pm[:, J:], (192, 256), records=([1, 2, 3, 4, 5], _xform(5)))
    assert (rec[:, 1] > 0).tolist() == [False, True, False, True, False]
    assert rec[:, 0].tolist() == [1, 2, 3, 4, 5] and (rec[[0, 2, 4], 1:] == 0).all()
    nobody = dev.parse_lowres(torch.zeros_like(R), Pm[:, J:], (192, 256), records=([9, 8, 7, 6, 5], None))
    lists = dev.parse_lowres(torch.zeros_like(R), Pm[:, J:], (192, 256))
    _equal(nobody, _host_records([9, 8, 7, 6, 5], lists))
    assert (nobody[:, 1:] == 0).all() and nobody[:, 0].tolist() == [9, 8, 7, 6, 5]


# ---- pipelines --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
def test_teacher_pipeline_records_equal_the_list_path(nat, teacher, flip):
    """five batches of 3 images whose records all differ: a buffer handed out again too early would show"""
    from rtpe.engine import RECORD_FLOATS, TeacherPipeline
    pipe = TeacherPipeline(teacher, _parser(), device=DEV, flip_test=flip, match_on="device")
    batches = [synth.make_images(3, 128, 160, seed=70 + k).to(DEV) for k in range(5)]
    ids = [[100 * k + i for i in range(3)] for k in range(5)]
    xf = [_xform(3, seed=k) if k % 2 else None for k in range(5)]
    asked = []

    def records(k):
        asked.append(k)
        return ids[k], xf[k]
    got = list(pipe.stream(iter(batches), records=records))
    assert _turns(pipe.parser) == {}                            # five batches in flight, no ring buffer taken
    torch.cuda.synchronize()
    lists = list(pipe.stream(iter(batches)))
    turns = _turns(pipe.parser)
    assert turns and any(turns.values())                        # (the list path does take them: 5 batches, rings of 4)
    assert asked == [0, 1, 2, 3, 4] and len(got) == len(lists) == 5
    for k in range(5):
        want = _host_records(ids[k], lists[k], xf[k])
        assert tuple(got[k].shape) == (3, RECORD_FLOATS)
        _equal(got[k], want)
        _equal(pipe(batches[k], image_ids=ids[k], xform=xf[k]), want)
    assert _turns(pipe.parser) == turns
    assert sum(_n(p) for r in lists for p, _ in r) >= 5
    for a in range(5):
        for b in range(a + 1, 5):
            assert not torch.equal(got[a][:, 1:], got[b][:, 1:])       # (column 0: the ids differ anyway)
    # the stream that was current is made to wait on the device: used at once, no host wait in between
    sums = [r.sum(dtype=torch.float64) for r in pipe.stream(iter(batches), records=records)]
    assert _turns(pipe.parser) == turns
    for k in range(5):
        assert float(sums[k]) == float(got[k].sum(dtype=torch.float64))


def test_student_pipeline_records_equal_the_list_path(nat, stream_case):  # noqa: F811
    from rtpe.engine import StudentPipeline
    dets, xs, _ = stream_case
    dets, xs, hws = dets[:3], xs[:3], STREAM_HW[:3]             # (three: the two-step delay, both workspace slots)
    ids = [[11, 12, 13, 14], [21, 22, 23, 24], [31, 32, 33, 34]]
    xf = [None, _xform(4), None]
    got = list(StudentPipeline(_StandIn(dets), _parser(), DEV, match_on="device")
               .stream(iter(xs), out_hw=lambda k: hws[k], records=lambda k: (ids[k], xf[k])))
    lists = list(StudentPipeline(_StandIn(dets), _parser(), DEV, match_on="device")
                 .stream(iter(xs), out_hw=lambda k: hws[k]))
    call = StudentPipeline(_StandIn(dets), _parser(), DEV, match_on="device")
    assert len(got) == len(lists) == 3
    for k in range(3):
        want = _host_records(ids[k], lists[k], xf[k])
        _equal(got[k], want)
        _equal(call(xs[k], hws[k], image_ids=ids[k], xform=xf[k]), want)
    assert sum(_n(p) for r in lists for p, _ in r) >= 3
    assert not torch.equal(got[0][:, 1:], got[1][:, 1:])


def test_multi_scale_pipeline_streamed_records_equal_those_of_the_call(nat, teacher):
    """three batches (the two-step delay, both workspace slots), every batch with ids of its own: the record tensor
    that the loop yields for batch k is the one ``pipe(batch_k, image_ids=ids_k)`` returns - ``records(k)`` reaches the
    grouping of batch k, two steps after it was asked for"""
    from rtpe.engine import RECORD_FLOATS
    pipe = _small_pipe(teacher, match_on="device")
    batches = _small_batches(3)
    ids = [[100 * k + i for i in range(2)] for k in range(3)]
    got = list(pipe.stream(iter(batches), in_flight=2, decode_stream="side", records=lambda k: (ids[k], None)))
    assert len(got) == 3
    for k in range(3):
        assert tuple(got[k].shape) == (2, RECORD_FLOATS) and got[k][:, 0].tolist() == ids[k]
        assert torch.equal(got[k], pipe(batches[k], image_ids=ids[k]))
    assert sum(float(g[:, 1].sum()) for g in got) >= 3
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.equal(got[a][:, 1:], got[b][:, 1:])       # (column 0: the ids differ anyway)


def test_records_are_refused_before_any_gpu_work(nat, teacher):
    from rtpe.engine import TeacherPipeline
    Pm, R, _, _ = _blob_outputs(2, 192, 256, seed=21)
    host, dev = _parser(), _parser(match_on="device")
    with pytest.raises(ValueError, match="match_on='device'"):
        host.parse_lowres(R, Pm[:, J:], (192, 256), records=([1, 2], None))
    st = host.lowres_topk(R, Pm[:, J:], (192, 256))
    with pytest.raises(ValueError, match="match_on='device'"):
        host.lowres_match(st, records=([1, 2], None))
    for rec, word in ((([1, (1 << 24) + 1], None), "2\\*\\*24"), (([1, 2, 3], None), "3 image ids for 2"),
                      (([1, 2], np.zeros((2, 5))), "xform"), (([1, 2], np.zeros((3, 6))), "xform")):
        with pytest.raises(ValueError, match=word):
            dev.parse_lowres(R, Pm[:, J:], (192, 256), records=rec)
        with pytest.raises(ValueError, match=word):
            dev.parse_flip(Pm, R, Pm, R, records=rec)
    calls = []
    pipe = TeacherPipeline(teacher, _parser(), device=DEV, match_on="host")
    pipe.model = lambda x: calls.append(1)                  # any forward would show
    x = torch.zeros((2, 3, 128, 160), device=DEV)
    with pytest.raises(ValueError, match="match_on='device'"):
        pipe(x, image_ids=[1, 2])
    with pytest.raises(ValueError, match="match_on='device'"):
        next(pipe.stream(iter([x]), records=lambda k: ([1, 2], None)))
    pipe.parser.match_on = "device"
    with pytest.raises(ValueError, match="2\\*\\*24"):
        pipe(x, image_ids=[1, (1 << 24) + 1])
    with pytest.raises(ValueError, match="1 image ids for 2"):
        next(pipe.stream(iter([x]), records=lambda k: ([1], None)))
    with pytest.raises(ValueError, match="xform"):
        pipe(x, image_ids=[1, 2], xform=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="goes with image_ids"):
        pipe(x, xform=np.zeros((2, 6)))
    assert not calls
    torch.cuda.synchronize()


# ---- gather -------------------------------------------------------------------------------------------------------------
def test_gather_of_a_record_tensor_over_rccl_one_rank(nat, teacher):
    """the pattern of test_rccl_collectives_on_device_tensors_one_rank: a one-rank ``nccl`` group in this process"""
    import socket
    import torch.distributed as dist
    from rtpe import engine
    assert not dist.is_initialized()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device(DEV))
    try:
        pipe = engine.TeacherPipeline(teacher, _parser(), device=DEV, match_on="device")
        x = synth.make_images(3, 128, 160, seed=70).to(DEV)
        ids = [11, 12, 13]
        rec = pipe(x, image_ids=ids)
        lists = pipe(x)
        for eq in (True, False):
            out = pipe.gather(None, rec, equal_counts=eq, force_collective=True)
            assert out.is_cuda and torch.equal(out, rec)
            want = engine.unpack_records(pipe.gather(ids, lists, equal_counts=eq, force_collective=True))
            got = engine.unpack_records(out)
            assert sorted(got) == sorted(want) == ids
            for i in ids:
                assert np.array_equal(got[i][0], want[i][0]) and np.array_equal(got[i][1], want[i][1])
        assert sum(len(v[1]) for v in got.values()) >= 1
        with pytest.raises(ValueError, match="image_ids=None"):
            pipe.gather(ids, rec, force_collective=True)
    finally:
        dist.destroy_process_group()


# ---- drivers ------------------------------------------------------------------------------------------------------------
def _driver_images():
    rng = np.random.default_rng(4)
    return [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in ((120, 160), (150, 200), (120, 160))]


def _driver_records(ids, results):
    """``pack_records`` of a driver's list result ``[(final_results, scores)]`` (``get_final_preds`` done on the host)"""
    from rtpe import engine
    lists = [(np.stack(f) if len(f) else np.array([], np.float32), s) for f, s in results]
    return engine.pack_records(ids, lists, "cpu"), sum(len(f) for f, _ in results)


def test_flip_test_inference_records(nat, teacher):
    from rtpe import inference
    images, ids = _driver_images(), [5, 581929, 0]
    kw = dict(input_size=128, batch_size=2, device=DEV, match_on="device")
    want, people = _driver_records(ids, inference.flip_test_inference(teacher, _parser(), images, **kw))
    _equal(inference.flip_test_inference(teacher, _parser(), images, image_ids=ids, **kw), want)
    assert people >= 1
    # device grouping set on the parser instead of asked for; the parser is not switched
    p = _parser(match_on="device")
    kw.pop("match_on")
    _equal(inference.flip_test_inference(teacher, p, images, image_ids=ids, **kw), want)
    assert p.match_on == "device"


@pytest.mark.parametrize("flip", [True, False])
def test_multi_scale_batch_inference_records(nat, teacher, flip):
    from rtpe import inference
    images, ids = _driver_images(), [5, 581929, 0]
    kw = dict(input_size=128, scale_factors=(1, 0.5), flip_test=flip, batch_size=2, device=DEV, match_on="device")
    want, people = _driver_records(ids, inference.multi_scale_batch_inference(teacher, _parser(), images, **kw))
    _equal(inference.multi_scale_batch_inference(teacher, _parser(), images, image_ids=ids, **kw), want)
    assert people >= 1


def test_plain_inference_records(nat, teacher):
    """images of one input size and different original sizes in one batch (per-image decode sizes), no transform"""
    from rtpe import inference
    images, ids = _driver_images(), [5, 581929, 0]
    kw = dict(input_size=128, batch_size=2, device=DEV, match_on="device")
    lists = inference.plain_inference(teacher, _parser(), images, **kw)
    p = _parser()
    _equal(inference.plain_inference(teacher, p, images, image_ids=ids, **kw), _host_records(ids, lists))
    assert p.match_on == "device" and _turns(p) == {}           # the per-image sizes table is no ring buffer either
    assert sum(_n(p) for p, _ in lists) >= 1
