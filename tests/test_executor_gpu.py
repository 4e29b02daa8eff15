"""The executor's entries around one forward (csrc/engine.hip: run() and its parts; run with -m gpu on an MI355X).

Two properties of run() that no kernel test sees:

  every entry runs the same forward   rtpe_hrnet_forward, _forward_flags (0 and RTPE_FWD_NO_LANES), _forward_timed and
                                      _forward_record give the same bits on one handle and one input - with lanes and on one
                                      stream, with per-op events and without - and the two per-op time vectors are well formed.
  a refused forward enqueues nothing  what check_ops() refuses is refused before the first launch: the workspace and both
                                      outputs, preset to a byte pattern, are untouched after the call, and the handle still
                                      computes what it computed before.

The entries are called through ctypes, so that the test owns every buffer.  The refusals are error returns; nothing faults."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERN = 0xA5
E_INVALID = -1                     # include/rtpe_hip.h
FWD_NO_LANES = 1
BLOCK_TAIL = -900002               # rtpe_hrnet_op_tile's mark of a fused BasicBlock's second conv


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


class Call:
    """one handle with caller-owned buffers for one shape: x, the two outputs and the workspace"""

    def __init__(self, nat, eng, N, H, W, x, aux=None):
        self.nat, self.L, self.eng, self.shape = nat, nat.lib(), eng, (N, H, W)
        self.x, self.aux = x.contiguous().to(DEV), None if aux is None else aux.float().contiguous().to(DEV)
        self.xdt = nat.RTPE_DTYPE_F16 if x.dtype == torch.float16 else nat.RTPE_DTYPE_F32
        (c0, d0), (c1, d1) = eng.program.outputs
        self.outs = [torch.empty((N, c, H >> d, W >> d), dtype=torch.float32, device=DEV) for c, d in ((c0, d0), (c1, d1))]
        need = ctypes.c_size_t()
        nat.check(self.L.rtpe_hrnet_workspace_bytes(eng._h, N, H, W, ctypes.byref(need)))
        self.ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=DEV)
        assert self.ws.data_ptr() % 256 == 0
        self.n_ops = len(eng.program.ops)

    def args(self, odt=None):
        N, H, W = self.shape
        return (self.eng._h, self.x.data_ptr(), self.xdt, N, H, W, self.outs[0].data_ptr(), self.outs[1].data_ptr(),
                self.nat.RTPE_DTYPE_F32 if odt is None else odt, self.ws.data_ptr(), self.ws.numel(),
                self.nat.stream_ptr(torch.device(DEV)))

    def args_aux(self, odt=None):
        a = self.args(odt)
        return a[:3] + (self.aux.data_ptr(),) + a[3:]

    def preset(self):
        for t in self.outs + [self.ws]:
            t.view(torch.uint8).fill_(PATTERN)

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t.view(torch.uint8) == PATTERN).all()) for t in self.outs + [self.ws])

    def result(self, rc):
        """the two outputs (numpy) of a forward that returned rc"""
        self.nat.check(rc)
        torch.cuda.synchronize()
        return [o.cpu().numpy().copy() for o in self.outs]

    def error(self):
        return self.L.rtpe_last_error_string().decode()


def _same(got, want, what):
    for g, w, name in zip(got, want, ("preds", "refined")):
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), "%s: %s differs" % (what, name)


# --------------------------------------------------------------------------- #
# every entry runs the same forward
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def teacher_engine(nat, w48_shapes):
    from rtpe.helpers import build_hrnet_w48_teacher
    sd = synth.make_state_dict(w48_shapes, 0, "W0")
    m = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(DEV)
    return m, m[1]._engine(torch.device(DEV))          # (the module keeps the engine alive)


def _times_ok(ms, tails, what):
    ms = np.array(ms, np.float64)
    assert ms.shape == (len(tails),), what
    assert np.isfinite(ms).all() and (ms >= 0).all(), (what, ms.min())
    assert (ms[tails] == 0.0).all(), (what, "a fused block's second conv has a time of its own")
    assert ms.sum() > 0, what


# N=2, 64 x 96: the fused block, the fused stem, the 1x1 pairs and the stride-2 group all route.  N=1, 32 x 32: the 1/4 map
# is 8 x 8, below the block kernel's 6 x 16, so both convs of every block of branch 0 launch on their own; the four blocks
# behind the transposed conv work on the 1/2 map, 16 x 16, and stay fused
@pytest.mark.parametrize("N,H,W", [(2, 64, 96), (1, 32, 32)], ids=["n2_64x96", "n1_32x32"])
def test_every_entry_runs_the_same_forward(nat, teacher_engine, N, H, W):
    _, eng = teacher_engine
    L = nat.lib()
    c = Call(nat, eng, N, H, W, synth.make_images(N, H, W, seed=7).half())
    marks = [eng.op_tile(i, N, H, W)[7] for i in range(c.n_ops)]
    tails = np.array([m == BLOCK_TAIL for m in marks])
    print("marks at %s: %s; %d second convs of fused blocks" % ((N, H, W), sorted(set(m for m in marks if m <= -100000)), tails.sum()))
    tails_64x96 = np.array([eng.op_tile(i, 2, 64, 96)[7] == BLOCK_TAIL for i in range(c.n_ops)])
    ds_in = np.array([eng.program.tensors[op.in_t].ds_log2 if op.in_t >= 0 else -1 for op in eng.program.ops])
    assert tails_64x96.sum() > 4 and set(ds_in[tails_64x96]) == {1, 2}          # (so the test cannot pass by routing nothing)
    if (H, W) == (32, 32):      # no block on the 1/4 map carries the mark: those second convs are launches of their own
        assert tails.sum() == 4 and set(ds_in[tails]) == {1} and not (tails & ~tails_64x96).any()
    else:
        assert np.array_equal(tails, tails_64x96)

    want = c.result(L.rtpe_hrnet_forward(*c.args()))
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.abs(want[0]).max() > 0
    for flags in (0, FWD_NO_LANES):
        c.preset()
        _same(c.result(L.rtpe_hrnet_forward_flags(*c.args(), flags)), want, "forward_flags(%d)" % flags)
    c.preset()
    ms = (ctypes.c_float * c.n_ops)(*([-1.0] * c.n_ops))
    _same(c.result(L.rtpe_hrnet_forward_timed(*c.args(), ms, c.n_ops)), want, "forward_timed")
    _times_ok(list(ms), tails, "forward_timed")
    c.preset()
    _same(c.result(L.rtpe_hrnet_forward_record(*c.args(), 3)), want, "forward_record")
    ms = (ctypes.c_float * c.n_ops)(*([-1.0] * c.n_ops))
    nat.check(L.rtpe_hrnet_read_record(eng._h, 3, ms, c.n_ops))
    _times_ok(list(ms), tails, "read_record")


# --------------------------------------------------------------------------- #
# a refused forward enqueues nothing
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def refusing(nat):
    """A program in which launching ops stand before every op that check_ops() refuses: the fp16 stem, the packed second
    input, two fp32 1x1 convs of it (the logits, the gated map), a sigmoid_add that emits its map as `preds`, and a head."""
    import torch.nn as nn
    from rtpe.third_party.pose_higher_hrnet import Engine, ProgramBuilder
    torch.manual_seed(5)
    b = ProgramBuilder(f32=False)
    b.stem(nn.Conv2d(3, 64, 3, 2, 1, bias=False).half(), nn.BatchNorm2d(64).eval())
    b.f32 = True
    a = b.aux_input()
    lg = b.conv(a, nn.Conv2d(4, 1, 1), None)
    x = b.conv(a, nn.Conv2d(4, 8, 1), None)
    y = b.sigmoid_add(lg, x, out_flag=nat.F_OUT_PREDS)
    b.conv(y, nn.Conv2d(b.tensors[y][0], 4, 1), None, out_flag=nat.F_OUT_REFINED, nhwc=False)
    prog = b.finish()
    kinds = [op.kind for op in prog.ops]
    assert kinds[0] == nat.OP_STEM and kinds.index(nat.OP_AUX_PACK) > 0 and kinds.index(nat.OP_SIGMOID_ADD) > 2
    eng = Engine(prog, 0)
    g = torch.Generator().manual_seed(6)
    c = Call(nat, eng, 1, 32, 32, torch.randn(1, 3, 32, 32, generator=g).half(), aux=torch.randn(1, 3, 32, 32, generator=g))
    want = c.result(c.L.rtpe_hrnet_forward_aux(*c.args_aux()))
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.abs(want[1]).max() > 0
    return c, want


def _refused(c, want, rc, text, code=E_INVALID):
    msg = c.error()
    assert rc == code and text in msg, (rc, msg)
    assert c.untouched(), "a refused forward wrote to the workspace or to an output (%s)" % msg
    _same(c.result(c.L.rtpe_hrnet_forward_aux(*c.args_aux())), want, "the forward after the refusal")


def test_a_forward_without_the_second_input_enqueues_nothing(refusing):
    c, want = refusing
    c.preset()
    _refused(c, want, c.L.rtpe_hrnet_forward(*c.args()), "second input")


def test_a_sigmoid_map_into_a_half_buffer_enqueues_nothing(refusing):
    c, want = refusing
    c.preset()
    _refused(c, want, c.L.rtpe_hrnet_forward_aux(*c.args_aux(c.nat.RTPE_DTYPE_F16)), "float32 buffer")


def test_a_timed_forward_with_too_few_times_enqueues_nothing(nat, teacher_engine):
    _, eng = teacher_engine
    c = Call(nat, eng, 1, 32, 32, synth.make_images(1, 32, 32, seed=8).half())
    want = c.result(c.L.rtpe_hrnet_forward(*c.args()))
    c.preset()
    ms = (ctypes.c_float * c.n_ops)()
    rc = c.L.rtpe_hrnet_forward_timed(*c.args(), ms, c.n_ops - 1)
    msg = c.error()
    assert rc == E_INVALID and "op_ms too small" in msg, (rc, msg)
    assert c.untouched(), "a refused forward wrote to the workspace or to an output"
    _same(c.result(c.L.rtpe_hrnet_forward(*c.args())), want, "the forward after the refusal")
