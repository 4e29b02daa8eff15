"""Real forwards are ordered: the happens-before checker (oracle/schedule.py) on traces of the executor (run with -m gpu
on an MI355X).

A traced forward (RTPE_FWD_TRACE, include/rtpe_hip_trace.h) reports what it enqueued; the checker derives what every
launch reads and writes from the descs and the route kinds and asks that every conflicting pair is ordered by stream
order, fork, join or an event recorded earlier in the same forward, and that no slot is handed on before its tensor's
last reader.  Nothing here tries to make a race happen: a missing edge is a finding whether or not the GPU would
have shown it.

Teacher (W48, the only program with regions), option "lanes" = 1, N = 1 at 64 x 64 and N = 2 at 64 x 96, one traced
forward per option set.  Each case asserts: no finding; `preds` and `refined` torch.equal to a RTPE_FWD_NO_LANES forward
of the same input; a lane stream launched at least one op.  The default trace is counted, so that clean cannot mean
empty: cross-lane read-after-write waits, grouped stride-2 launches, a pair tail with a projection folded from lane 1,
a region with work on all four streams.

Structures the real programs never contain, which tests/test_schedule_host.py covers with hand-built programs: a
cross-lane write-after-read (the only `into=` tensor, the concat of the last fuse output and head 0, is written on lane
0 and read behind the join), a 1x1 pair head inside a region whose output another lane reads, and a stride-2 group
member with a wait that the group's first op does not have too.

The students run on the caller's stream but for one op: the skip projection of layer1's first Bottleneck has a
region and a lane of its own in their programs too.  What is checked there is mostly the slot lifetimes against the
launches that actually happen (a 64 x 64, a ragged 33 x 47 and a mixed-size forward).

Launch shapes are the default ones (RTPE_AUTOTUNE=0 for this module): tuning changes tiles, not what a launch touches."""
import ctypes

import pytest
import torch

from oracle import schedule as S
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((1, 64, 64), (2, 64, 96))
OPTION_SETS = [("defaults", {}), ("pair_1x1=0", {"pair_1x1": 0}), ("pair_proj=0", {"pair_proj": 0}), ("conv48s2=0", {"conv48s2": 0}),
               ("fused_stem=0", {"fused_stem": 0}), ("fused_stem=1", {"fused_stem": 1}), ("fused_stem=2", {"fused_stem": 2}),
               ("block_pc=0", {"block_pc": 0}), ("head_direct=0", {"head_direct": 0}), ("deconv48=0", {"deconv48": 0}),
               ("direct_1x1=0", {"direct_1x1": 0})]


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    return _native


@pytest.fixture(autouse=True)
def default_launch_shapes(monkeypatch):
    monkeypatch.setenv("RTPE_AUTOTUNE", "0")


class Options:
    """sets executor options for a block and restores what they were"""

    def __init__(self, nat, **opts):
        self.nat, self.opts, self.prev = nat, opts, {}

    def __enter__(self):
        L = self.nat.lib()
        for k, v in self.opts.items():
            old = ctypes.c_int32()
            self.nat.check(L.rtpe_get_option(k.encode(), ctypes.byref(old)))
            self.prev[k] = old.value
            self.nat.check(L.rtpe_set_option(k.encode(), v))
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.nat.check(self.nat.lib().rtpe_set_option(k.encode(), v))


def traced(run):
    """run() under RTPE_FWD_TRACE and under RTPE_FWD_NO_LANES: (outputs of the traced forward, outputs on one stream)"""
    from rtpe.third_party import pose_higher_hrnet as phh
    outs = []
    for flags in (phh.FWD_TRACE, phh.FWD_NO_LANES):
        prev = phh.set_forward_flags(flags)
        try:
            with torch.no_grad():
                outs.append([t.clone() for t in run()])
        finally:
            phh.set_forward_flags(prev)
    torch.cuda.synchronize()
    return outs


def check_forward(eng, run, what, lanes=True):
    got, want = traced(run)
    trace = eng.read_trace()           # (the one-stream forward is not traced: the kept trace is the first forward's)
    ops, tensors = S.descs(eng.program)
    assert sum(1 for r in trace if r[0] == S.LAUNCH) == len(ops), what
    for g, w, name in zip(got, want, ("preds", "refined")):
        assert torch.isfinite(w).all() and float(w.abs().max()) > 0, (what, name)
        assert torch.equal(g, w), "%s: %s of the traced forward differs from the one-stream forward" % (what, name)
    findings = S.check(ops, tensors, trace)
    assert findings == [], (what, len(findings), [f["text"] for f in findings[:8]])
    st = S.structure(ops, tensors, trace)
    # every op of a lane ran on that lane's stream, every other op on the caller's
    for r in trace:
        if r[0] == S.LAUNCH:
            assert r[2] == (ops[r[1]]["lane"] if ops[r[1]]["region"] > 0 else 0), (what, r)
    if lanes:
        assert st["lane_launches"] >= 1, (what, st)
    return ops, tensors, trace, st


def _teacher(w48_shapes, f32=False):
    from rtpe.helpers import build_hrnet_w48_teacher
    sd = synth.make_state_dict(w48_shapes, 0, "W0")
    m = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()})
    if f32:
        m = m.float()
    m = m.to(DEV)
    return m, m[1]._engine(torch.device(DEV))


@pytest.fixture(scope="module")
def teacher(nat, w48_shapes):
    return _teacher(w48_shapes)          # (the module keeps the engine alive)


def _images(N, H, W, f32=False):
    x = synth.make_images(N, H, W, seed=7).to(DEV)
    return x if f32 else x.half()


@pytest.mark.parametrize("name,opts", OPTION_SETS, ids=[n for n, _ in OPTION_SETS])
def test_teacher_forwards_are_ordered(nat, teacher, name, opts):
    _, eng = teacher
    with Options(nat, lanes=1, **opts) as o:
        for N, H, W in SHAPES:
            x = _images(N, H, W)
            ops, tensors, trace, st = check_forward(eng, lambda: eng.forward(x), "%s at %dx%dx%d" % (name, N, H, W))
            print("%s %s: %s" % (name, (N, H, W), st))
            routes = S.routes_of(trace, len(ops))
            kinds = set(how for how, _ in routes)
            if name == "defaults" and (N, H, W) == SHAPES[0]:
                # the structure counts: a clean result is not a vacuous one
                assert st["raw_waits"] >= 1 and st["s2_groups"] >= 1 and st["proj_from_lane1"] >= 1 and st["regions_4_streams"] >= 1, st
                assert st["war_waits"] == 0, st              # (see the module docstring: host tests cover it)
                assert {S.ROUTE_BLOCK, S.ROUTE_PAIR_TAIL, S.ROUTE_PAIR_PROJ, S.ROUTE_S2_GROUP, S.ROUTE_STEM_FUSED} <= kinds, kinds
            # the option did what its name says to the routes (so each case checks another schedule)
            if name == "pair_1x1=0":
                assert not kinds & {S.ROUTE_PAIR_HEAD, S.ROUTE_PAIR_TAIL, S.ROUTE_PAIR_PROJ}
            if name == "pair_proj=0":
                assert S.ROUTE_PAIR_PROJ not in kinds and S.ROUTE_PAIR_TAIL in kinds
            if name == "conv48s2=0":
                assert not kinds & {S.ROUTE_S2, S.ROUTE_S2_GROUP}
            if name in ("fused_stem=0", "fused_stem=2"):
                assert S.ROUTE_STEM_FUSED not in kinds and (S.ROUTE_STEM_PLAIN if name[-1] == "0" else S.ROUTE_STEM_CONV1) in kinds
            if name == "head_direct=0":
                assert S.ROUTE_HEAD not in kinds
            if name == "deconv48=0":
                assert S.ROUTE_DECONV_MERGED + 1 not in kinds
        prev = dict(o.prev)
    for k, v in prev.items():
        got = ctypes.c_int32()
        nat.check(nat.lib().rtpe_get_option(k.encode(), ctypes.byref(got)))
        assert got.value == v, (k, got.value, v)


def test_fp32_teacher_forwards_are_ordered(nat, w48_shapes):
    m, eng = _teacher(w48_shapes, f32=True)
    assert eng.program.f32
    with Options(nat, lanes=1):
        for N, H, W in SHAPES:
            x = _images(N, H, W, f32=True)
            _, _, _, st = check_forward(eng, lambda: eng.forward(x), "fp32 teacher at %dx%dx%d" % (N, H, W))
            print("fp32 teacher %s: %s" % ((N, H, W), st))
    del m


@pytest.mark.parametrize("switch", ["_WIDE_REGIONS", "_S2_SIBLINGS"])
def test_teacher_forwards_are_ordered_with_a_program_switch_flipped(nat, w48_shapes, monkeypatch, switch):
    """the switches are module globals that emit() reads when a program is compiled: a model built and compiled with the
    global flipped gets the other program (the environment variable only sets the global's value at import)"""
    from rtpe.third_party import pose_higher_hrnet as phh
    base = S.descs(_teacher(w48_shapes)[1].program)[0]
    assert getattr(phh, switch) is True
    monkeypatch.setattr(phh, switch, False)
    m, eng = _teacher(w48_shapes)
    ops = S.descs(eng.program)[0]
    order = lambda o: [(d["in_t"], d["out_t"], d["lane"], d["region"]) for d in o]
    assert order(ops) != order(base), "flipping %s left the program as it was" % switch
    with Options(nat, lanes=1):
        for N, H, W in SHAPES:
            x = _images(N, H, W)
            _, _, trace, st = check_forward(eng, lambda: eng.forward(x), "%s flipped at %dx%dx%d" % (switch, N, H, W))
            print("%s=0 %s: %s" % (switch, (N, H, W), st))
            if switch == "_S2_SIBLINGS":
                assert st["s2_groups"] == 0, st
            else:
                assert st["proj_from_lane1"] == 0, st
    del m


# --------------------------------------------------------------------------- #
# the students: one stream, slot lifetimes against the launches that happen
# --------------------------------------------------------------------------- #
def _student(body_half):
    from rtpe.students import AttentionStudent
    torch.manual_seed(3)
    return AttentionStudent(None, "cpu", 100, 17, 1, True, None, False, body_half=body_half).eval().to(DEV)


@pytest.mark.parametrize("body_half", [False, True], ids=["fp32_body", "half_body"])
def test_student_forwards_keep_their_slot_lifetimes(nat, body_half):
    stu = _student(body_half)
    eng = stu._engine(torch.device(DEV))
    for N, H, W in ((1, 64, 64), (1, 33, 47)):
        x = synth.make_images(N, H, W, seed=11).to(DEV)
        _, _, trace, st = check_forward(eng, lambda: eng.forward(x.float(), torch.float32), "student %dx%d" % (H, W), lanes=False)
        print("student half=%s %s: %s" % (body_half, (H, W), st))
    # a mixed-size batch of two images: the forward ends with the launch that masks the outputs
    from rtpe.students import pack_mixed
    canvas, sizes = pack_mixed([synth.make_images(1, 33, 47, seed=12)[0].to(DEV), synth.make_images(1, 64, 40, seed=13)[0].to(DEV)])
    _, _, trace, st = check_forward(eng, lambda: eng.forward_mixed(canvas.float(), sizes), "student mixed", lanes=False)
    assert trace[-1][0] == S.MASK and sum(1 for r in trace if r[0] == S.MASK) == 1


def test_student_steps_forward_keeps_its_slot_lifetimes(nat):
    from rtpe.students import AttentionStudentSteps
    torch.manual_seed(4)
    stu = AttentionStudentSteps(None, "cpu", 48, 17, 1, True, None, False).eval().to(DEV)
    eng = stu._engine(torch.device(DEV), ("att_divisor", None))
    assert eng.program.has_aux
    x = synth.make_images(1, 64, 64, seed=14).to(DEV)
    alt = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(15)).to(DEV)
    _, _, _, st = check_forward(eng, lambda: eng.forward(x.float(), torch.float32, aux=alt), "student steps 64x64", lanes=False)
    print("student steps: %s" % st)
