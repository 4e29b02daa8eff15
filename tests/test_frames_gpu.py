"""The students' frames front end on an MI355X (run with -m gpu): ``students.pack_frames`` (one upload, one launch of
``rtpe_frames_to_canvases``) against the path it replaces, bit for bit.

The "old path" inputs are made on the CPU (tests/test_frames_host.py: ``to_tensor32``, ``normalized32`` - torch-CPU's
``to_tensor`` + ``Normalize`` bit for bit) and uploaded; the alt images are today's ``dataloaders.rgb2lab`` / ``rgb2hsv``
of the uploaded ``to_tensor`` image.  Every output canvas lies between guard bands and is preset to a NaN pattern, so an
element the kernel does not write shows, and so does one it writes outside.  All comparisons are of bits, except LAB
against the float64 restatement (2e-3, the bound of test_alt_colour_spaces_on_the_gpu)."""
import ctypes

import numpy as np
import pytest
import torch

import test_frames_host as H
from oracle import exact, student_ref, synth
from test_student_pipeline_gpu import _det, _n_people, _parser
from test_student_pipeline_gpu import _same as _same_people

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [None, "LAB", "HSV"]


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


@pytest.fixture(autouse=True)
def default_launch_shapes(monkeypatch):
    monkeypatch.setenv("RTPE_AUTOTUNE", "0")


# --------------------------------------------------------------------------- #
# the old path, computed once per frame
# --------------------------------------------------------------------------- #
_OLD = {}


def _old(frame):
    """frame -> {"t": to_tensor (3,h,w) on the GPU, made on the CPU; "x": Normalize of it, likewise; "LAB" / "HSV": today's
    kernel on "t"} - what a caller hands to ``call_mixed`` today"""
    from rtpe import dataloaders
    key = (frame.shape, frame.tobytes())
    if key not in _OLD:
        t = torch.from_numpy(np.ascontiguousarray(H.to_tensor32(frame).transpose(2, 0, 1))).to(DEV)
        _OLD[key] = {"t": t, "x": torch.from_numpy(H.normalized32(frame)).to(DEV),
                     "LAB": dataloaders.rgb2lab(t), "HSV": dataloaders.rgb2hsv(t)}
    return _OLD[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _pack_checked(frames, cs, canvas_hw=None, give=None, want_frames=None):
    """pack_frames into guarded NaN-preset canvases, every check of the canvases -> (canvas, alt_canvas) numpy"""
    from rtpe.students import pack_frames
    want_frames = frames if want_frames is None else want_frames
    N = len(want_frames)
    Hc, Wc = canvas_hw or (max(f.shape[0] for f in want_frames), max(f.shape[1] for f in want_frames))
    go = exact.guarded_out((N, 3, Hc, Wc), torch.float32)
    ga = exact.guarded_out((N, 3, Hc, Wc), torch.float32) if cs else None
    spare = exact.guarded_out((N, 3, Hc, Wc), torch.float32)          # passed nowhere
    assert bool(torch.isnan(go.t).all()) and go.t.is_contiguous()
    canvas, sizes, alt = pack_frames(frames if give is None else give, cs, canvas_hw, out=(go.t, ga.t if cs else None))
    torch.cuda.synchronize()
    assert canvas is go.t and (alt is None if cs is None else alt is ga.t)
    assert sizes == [f.shape[:2] for f in want_frames]
    assert exact.guards_intact(go, ga, spare), "a guard band was overwritten"
    assert bool((spare.t.view(torch.int32) == spare.bits).all()), "a tensor that was passed nowhere was written"
    c = canvas.cpu().numpy()
    a = alt.cpu().numpy() if cs else None
    inside = np.zeros(c.shape, bool)
    for n, f in enumerate(want_frames):
        h, w = f.shape[:2]
        inside[n, :, :h, :w] = True
        what = "image %d (%d x %d) in a %d x %d canvas, %s" % (n, h, w, Hc, Wc, cs)
        want = H.normalized32(f)
        assert np.array_equal(_bits(c[n, :, :h, :w]), _bits(want)), what + ": " + exact.first_differences(
            np.ascontiguousarray(c[n, :, :h, :w]), want)
        if cs:
            old = _old(f)[cs].cpu().numpy()
            got = np.ascontiguousarray(a[n, :, :h, :w])
            assert np.array_equal(_bits(got), _bits(old)), what + ": " + exact.first_differences(got, old)
            t = H.to_tensor32(f)
            if cs == "HSV":
                assert np.array_equal(got, H.hsv32(t)), what + ": the float32 oracle"
            else:
                ref = student_ref.rgb2lab(t).transpose(2, 0, 1)
                err = float(np.abs(got - ref).max())
                print("%s: LAB max err %.2e vs float64" % (what, err))
                assert err <= 2e-3, what
    for name, m in (("canvas", c), ("alt canvas", a)):
        if m is not None:
            assert not np.isnan(m).any(), name
            assert bool((_bits(m)[~inside] == 0).all()), "%s: an element outside every image is not 0.0" % name
    return c, a


# --------------------------------------------------------------------------- #
# canvases
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("cs", MODES, ids=str)
@pytest.mark.parametrize("canvas_hw", H.OP_CANVASES, ids=lambda c: "default" if c is None else "%dx%d" % c)
def test_101_three_sizes_in_two_canvases(nat, canvas_hw, cs):
    frames = H.seeded_frames()
    c, a = _pack_checked(frames, cs, canvas_hw)
    assert c.shape == (3, 3) + (canvas_hw or (64, 47))
    assert float(np.abs(c).max()) > 1 and (a is None or float(np.abs(a).max()) > 0)


@pytest.mark.parametrize("cs", MODES, ids=str)
def test_102_all_levels(nat, cs):
    """every grey level through both branches of the linearisation, d == 0, each hue branch, the hue's wrap: what a
    table of the linearisation can get wrong.  One frame wider than a workgroup's 256 columns would hide a fault of the
    second workgroup in x: the second frame is 40 x 300"""
    wide = np.random.default_rng(5).integers(0, 256, (40, 300, 3), dtype=np.uint8)
    _pack_checked([H.all_levels_frame(), wide], cs)


def test_103_the_same_frames_given_five_ways(nat):
    from rtpe.students import pack_frames
    frames = H.seeded_frames()
    want = [_pack_checked(frames, cs) for cs in ("LAB", "HSV")]

    def wide(f):                                 # a crop of a wider image: row stride > 3 * w, odd start address
        h, w = f.shape[:2]
        big = torch.zeros((h + 2, w + 7, 3), dtype=torch.uint8, device=DEV)
        big[1:h + 1, 3:w + 3] = torch.from_numpy(f).to(DEV)
        view = big[1:h + 1, 3:w + 3]
        assert view.stride(0) == 3 * (w + 7) and not view.is_contiguous()
        return view
    ways = {"ndarrays": lambda f, n: f,
            "cpu tensors": lambda f, n: torch.from_numpy(f),
            "device tensors": lambda f, n: torch.from_numpy(f).to(DEV),
            "strided device views": lambda f, n: wide(f),
            "mixed": lambda f, n: [f, wide(f), torch.from_numpy(f)][n],
            "a BGR-flipped view of a host array": lambda f, n: np.ascontiguousarray(f[:, :, ::-1])[:, :, ::-1],
            # (pixel stride h * w, not 3: the one case that is made contiguous)
            "HWC views of CHW device tensors": lambda f, n: torch.from_numpy(
                np.ascontiguousarray(f.transpose(2, 0, 1))).to(DEV).permute(1, 2, 0)}
    for name, way in ways.items():
        give = [way(f, n) for n, f in enumerate(frames)]
        for (wc, wa), cs in zip(want, ("LAB", "HSV")):
            c, a = _pack_checked(frames, cs, give=give)
            assert np.array_equal(_bits(c), _bits(wc)) and np.array_equal(_bits(a), _bits(wa)), name
    # one (N, H, W, 3) tensor equals the list of its frames; fresh canvases (no out=) hold the same bits
    same = np.random.default_rng(9).integers(0, 256, (3, 40, 52, 3), dtype=np.uint8)
    wc, wa = _pack_checked(list(same), "LAB")
    for stack in (same, torch.from_numpy(same), torch.from_numpy(same).to(DEV)):
        c, a = _pack_checked(None, "LAB", give=stack, want_frames=list(same))
        assert np.array_equal(_bits(c), _bits(wc)) and np.array_equal(_bits(a), _bits(wa))
    canvas, sizes, alt = pack_frames(same, "LAB")
    assert canvas.shape == (3, 3, 40, 52) and np.array_equal(_bits(canvas.cpu().numpy()), _bits(wc))
    assert np.array_equal(_bits(alt.cpu().numpy()), _bits(wa))
    canvas, sizes, alt = pack_frames(frames)
    assert alt is None and np.array_equal(_bits(canvas.cpu().numpy()), _bits(want[0][0]))


def test_104_ring_reuse(nat):
    """more calls than the staging ring has slots, each with other data and another N, nothing waited for in between:
    all results checked after the last call"""
    from rtpe.students import pack_frames
    from rtpe.third_party import transforms
    calls = transforms.WARP_RING_SLOTS * 2 + 1
    sets, got = [], []
    for k in range(calls):
        sizes = [(32 + (5 * k + 11 * i) % 40, 32 + (7 * k + 3 * i) % 50) for i in range(1 + k % 4)]
        sets.append(H.seeded_frames(sizes, seed=100 + k))
        got.append(pack_frames(sets[-1], "HSV"))
    torch.cuda.synchronize()
    for frames, (canvas, sizes, alt) in zip(sets, got):
        assert canvas.shape[0] == len(frames)
        for n, f in enumerate(frames):
            h, w = f.shape[:2]
            assert np.array_equal(_bits(canvas[n, :, :h, :w].cpu().numpy()), _bits(H.normalized32(f)))
            assert np.array_equal(alt[n, :, :h, :w].cpu().numpy(), H.hsv32(H.to_tensor32(f)))


# --------------------------------------------------------------------------- #
# pipeline
# --------------------------------------------------------------------------- #
class _Blob(torch.nn.Module):
    """runs the real student on what the pipeline hands it, keeps a copy of every input and output of ``forward_mixed``
    (the comparison of the two paths), and hands out prepared blob-bearing det maps instead of its own: seeded networks
    find no people"""

    def __init__(self, stu, dets, with_alt):
        super().__init__()
        self.stu, self.dets, self.seen = stu, dets, []
        if with_alt:
            self.forward_mixed = self._forward_mixed_alt

    def _lay(self, canvas, sizes, alt, out):
        att, det = out
        self.seen.append((canvas.clone(), None if alt is None else alt.clone(), att.clone(), det.clone()))
        det = det.clone()
        for n, hw in enumerate(sizes):
            d = self.dets[tuple(hw)]
            det[n, :, :d.shape[2], :d.shape[3]] = d[0]
        return att, det

    def forward_mixed(self, canvas, sizes):
        return self._lay(canvas, sizes, None, self.stu.forward_mixed(canvas, sizes))

    def _forward_mixed_alt(self, canvas, sizes, alt=None):
        return self._lay(canvas, sizes, alt, self.stu.forward_mixed(canvas, sizes, alt=alt))


def _pipe(golden_dir, which, match_on):
    from rtpe.engine import StudentPipeline
    from test_steps_mixed_gpu import _steps48
    from test_student_mixed_gpu import _student100
    dets = {hw: _det((-(-hw[0] // 4), -(-hw[1] // 4)), (51 + i,)).to(DEV) for i, hw in enumerate(H.OP_SIZES)}
    stu = _steps48(golden_dir) if which == "steps" else _student100(golden_dir, which == "half_body")
    return StudentPipeline(_Blob(stu, dets, which == "steps"), _parser(match_on), DEV)


def _same_seen(a, b, what):
    assert len(a) == len(b) == 4
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u, v), "%s: %s differs" % (
            what, ("canvas", "alt canvas", "att", "det")[i])


WHICH = pytest.mark.parametrize("which", ["fp32_body", "half_body", "steps"])


@WHICH
@pytest.mark.parametrize("decode", ["batch", "per_image"])
@pytest.mark.parametrize("match_on", ["host", "device"])
def test_201_call_frames_equals_call_mixed_on_old_path_inputs(nat, golden_dir, which, match_on, decode):
    pipe = _pipe(golden_dir, which, match_on)
    frames = H.seeded_frames()
    cs = "LAB" if which == "steps" else None
    old = [_old(f) for f in frames]
    kw = {"alt": [o["LAB"] for o in old]} if cs else {}
    want = pipe.call_mixed([o["x"] for o in old], decode=decode, **kw)
    got = pipe.call_frames(frames, alt_colorspace=cs, decode=decode)
    assert len(pipe.model.seen) == 2 and len(got) == len(want) == 3
    _same_seen(pipe.model.seen[0], pipe.model.seen[1], "call_frames vs call_mixed")
    assert float(pipe.model.seen[1][3].abs().max()) > 0
    for g, w in zip(got, want):
        _same_people(g, w)
    assert sum(_n_people(g[0]) for g in got) >= 1, "every decode came back empty"
    if match_on == "device":
        rec_w = pipe.call_mixed([o["x"] for o in old], image_ids=[7, 8, 9], decode=decode, **kw)
        rec_g = pipe.call_frames(frames, alt_colorspace=cs, image_ids=[7, 8, 9], decode=decode)
        for g, w in zip(rec_g, rec_w):
            assert torch.equal(g, w)
    torch.cuda.synchronize()


@WHICH
@pytest.mark.parametrize("in_flight", [1, 2])
def test_202_stream_frames_equals_call_frames_per_batch(nat, golden_dir, which, in_flight):
    from rtpe.engine import StudentPipeline
    pipe = _pipe(golden_dir, which, "host")
    frames = H.seeded_frames()
    cs = "LAB" if which == "steps" else None
    batches = [frames, [frames[2], torch.from_numpy(frames[0]).to(DEV)]]
    want = [pipe.call_frames(b, alt_colorspace=cs) for b in batches]
    seen_call = list(pipe.model.seen)
    del pipe.model.seen[:]
    got = list(pipe.stream_frames(iter(batches), alt_colorspace=cs, in_flight=in_flight))
    assert len(got) == 2 and len(pipe.model.seen) == 2
    for k in range(2):
        _same_seen(pipe.model.seen[k], seen_call[k], "stream_frames batch %d" % k)
        assert len(got[k]) == len(want[k]) == len(batches[k])
        for g, w in zip(got[k], want[k]):
            _same_people(g, w)
    # what frame_batches cuts goes straight in, and restore gives the caller's order back
    cut, restore = StudentPipeline.frame_batches(frames, batch_size=2)
    back = restore(list(pipe.stream_frames(iter(cut), alt_colorspace=cs, in_flight=in_flight)))
    for n in range(3):
        _same_people(back[n], want[0][n])
    torch.cuda.synchronize()


def test_203_the_half_steps_student(nat):
    """``call_frames`` keeps the mixed-batch refusal of AttentionStudentStepsHalf; frames of one size are a plain batch,
    which it takes as any tensor: the bits of the forward and the decode on old-path inputs"""
    from rtpe.engine import StudentPipeline
    from rtpe.students import pack_frames
    from test_steps_half_gpu import _half_steps
    stu = _half_steps(48, 4)
    pipe = StudentPipeline(stu, _parser(), DEV)
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        pipe.call_frames(H.seeded_frames(), alt_colorspace="LAB")
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        pipe.stream_frames(iter([H.seeded_frames()]), alt_colorspace="LAB")
    frames = H.seeded_frames([(96, 128), (96, 128)], seed=3)
    old = [_old(f) for f in frames]
    x, alt = torch.stack([o["x"] for o in old]), torch.stack([o["LAB"] for o in old])
    canvas, sizes, alt_canvas = pack_frames(frames, "LAB")
    assert torch.equal(canvas, x) and torch.equal(alt_canvas, alt) and sizes == [(96, 128)] * 2
    with torch.no_grad():
        want_maps = [t.clone() for t in stu(x, alt=alt)]
        got_maps = stu(canvas, alt=alt_canvas)
    assert torch.equal(got_maps[0], want_maps[0]) and torch.equal(got_maps[1], want_maps[1])
    assert float(want_maps[1].abs().max()) > 0
    want = pipe(x, alt=alt)
    got = pipe(canvas, alt=alt_canvas)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        _same_people(g, w)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- #
# refusals of the C side, before the launch
# --------------------------------------------------------------------------- #
def test_301_c_side_refusals_launch_nothing(nat):
    from rtpe.students import pack_frames
    L = nat.lib()
    frames = H.seeded_frames()
    tb = ctypes.c_size_t()
    nat.check(L.rtpe_frames_table_bytes(3, ctypes.byref(tb)))
    srcs = [torch.from_numpy(f).to(DEV) for f in frames]
    host = np.zeros(tb.value, np.uint8)
    nat.check(L.rtpe_frames_table_fill((ctypes.c_uint64 * 3)(*[s.data_ptr() for s in srcs]),
                                       (ctypes.c_int32 * 9)(*[v for f in frames for v in (f.shape[0], f.shape[1], 3 * f.shape[1])]),
                                       3, 64, 47, ctypes.c_void_p(host.ctypes.data), tb.value))
    table = torch.from_numpy(host).to(DEV)
    go, ga = exact.guarded_out((3, 3, 64, 47), torch.float32), exact.guarded_out((3, 3, 64, 47), torch.float32)
    got = H.launch_refusals(L, ctypes.c_void_p(table.data_ptr()), ctypes.c_void_p(go.t.data_ptr()),
                            ctypes.c_void_p(ga.t.data_ptr()))
    torch.cuda.synchronize()
    assert len(got) == 15
    for kw, rc in got:
        assert rc == -1, kw                                                  # RTPE_E_INVALID
    for g in (go, ga):
        assert bool((g.t.view(torch.int32) == g.bits).all()), "a refused call wrote"
    assert exact.guards_intact(go, ga)
    # and the accepted call with the same table and canvases after all of them: what pack_frames gives
    f3 = ctypes.c_float * 3
    nat.check(L.rtpe_frames_to_canvases(ctypes.c_void_p(table.data_ptr()), 3, 64, 47, f3(*H.MEAN), f3(*H.STD), 1,
                                        ctypes.c_void_p(go.t.data_ptr()), ctypes.c_void_p(ga.t.data_ptr()),
                                        nat.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    canvas, _, alt = pack_frames(frames, "HSV")
    assert torch.equal(go.t, canvas) and torch.equal(ga.t, alt) and exact.guards_intact(go, ga)
