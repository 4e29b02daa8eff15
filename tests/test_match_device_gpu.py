"""Grouping by tag on the GPU (csrc/match_dev.hip, HeatmapParser(match_on="device")): bit-identical to the host
matcher (csrc/match_host.cpp, itself pinned on the reference's match_by_tag run with the real munkres package) at the
table level - ans, person_img, counts and total - and, through every batch decode (parse_lowres, parse_flip,
parse_multi_scale with and without ags, TeacherPipeline call and stream), at the level of the final people and scores.
The yardstick is always the host path in the same process; no case is skipped or left out."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import synth
from test_ags_decode_gpu import _ags_outputs
from test_flip_decode_gpu import _assert_same, _blob_outputs
from test_multiscale_decode_gpu import H, W, _scale_outputs

pytestmark = pytest.mark.gpu

J, K = 17, 30
# max_num_people, detection_threshold, tag_threshold, use_detection_val, ignore_too_much
DEFAULT = (30, 0.1, 1.0, True, False)


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
    return build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to("cuda:0")


def _parser(cfg=DEFAULT, match_on="host", **kw):
    from rtpe.third_party.group import HeatmapParser
    return HeatmapParser(J, *cfg, match_on=match_on, **kw)


def _ind(loc):
    from rtpe.third_party.group import _W_ENC
    loc = np.asarray(loc)
    return (loc[..., 1].astype(np.int64) * _W_ENC + loc[..., 0].astype(np.int64)).astype(np.int32)


def _check_tables(cfg, tag, ind, val):
    """tag (N,J,K,D), ind (N,J,K), val (N,J,K): the four outputs of the kernel against the host matcher's; returns
    counts"""
    from rtpe.third_party.group import _W_ENC, _match_batch
    parser = _parser(cfg)
    flat, pimg, counts = _match_batch(tag, ind, val, _W_ENC, parser.params)
    ans, pimg_d, counts_d, total = parser.match_device(torch.from_numpy(np.ascontiguousarray(tag, np.float32)),
                                                       torch.from_numpy(np.ascontiguousarray(ind, np.int32)),
                                                       torch.from_numpy(np.ascontiguousarray(val, np.float32)), _W_ENC)
    assert ans.is_cuda and pimg_d.is_cuda and counts_d.is_cuda and total.is_cuda
    N, Jn, Kn, D = tag.shape
    assert tuple(ans.shape) == (N * Jn * Kn, Jn, 3 + D) and tuple(pimg_d.shape) == (N * Jn * Kn,)
    T = int(total.cpu()[0])
    got_counts = counts_d.cpu().numpy()
    assert np.array_equal(got_counts, counts), (got_counts, counts)
    assert T == int(counts.sum()) == flat.shape[0]
    assert np.array_equal(pimg_d[:T].cpu().numpy(), pimg)
    got = ans[:T].cpu().numpy()
    assert got.shape == flat.shape and got.dtype == flat.dtype
    assert np.array_equal(got.view(np.uint32), flat.view(np.uint32))      # the bits (NaN-proof, signed zeros)
    return counts


def _golden_match_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "match_vectors.npz"))
    cases = []
    for i in range(int(g["n_cases"])):
        mp, udv, itm = [int(v) for v in g["c%d_cfg" % i]]
        cases.append(((mp, 0.1, 1.0, bool(udv), bool(itm)), g["c%d_tag" % i], _ind(g["c%d_loc" % i]), g["c%d_val" % i]))
    return cases


def _golden_decode_cases(golden_dir):
    cases = []
    for name in ["p0", "p1", "p3", "p10", "p30", "p3_480", "p5_d2", "p40"]:
        g = np.load(os.path.join(golden_dir, "decode_%s.npz" % name))
        cases.append((DEFAULT, g["tag_k"][0], _ind(g["loc_k"][0]), g["val_k"][0]))
    return cases


def _generated_cases():
    """the generator of tests/test_host_logic.py::test_match_by_tag_variants_against_oracle (every D it draws - 1, 2 and
    9 - is supported by the kernel)"""
    rng = np.random.default_rng(9)
    cases = []
    for trial in range(40):
        D = int(rng.choice([1, 1, 2, 9]))
        val = np.sort(rng.random((J, K)).astype(np.float32) * (0.3 if trial % 3 else 1.0), axis=1)[:, ::-1]
        loc = rng.integers(0, 640, (J, K, 2)).astype(np.int64)
        tag = (rng.integers(0, 6, (J, K, D)) * 1.5 + rng.normal(0, 0.3, (J, K, D))).astype(np.float32)
        for cfg in (DEFAULT, (30, 0.1, 1.0, False, False), (5, 0.1, 1.0, True, True), (8, 0.1, 1.0, True, False)):
            cases.append((cfg, tag, _ind(loc), np.ascontiguousarray(val)))
    return cases


def _one_by_one(cases):
    counts = []
    for cfg, tag, ind, val in cases:
        counts.append(int(_check_tables(cfg, tag[None], ind[None], val[None])[0]))
    return counts


def test_match_device_golden_match_vectors(nat, golden_dir):
    cases = _golden_match_cases(golden_dir)
    assert len(cases) == 48 and {c[1].shape[2] for c in cases} == {1, 2}
    counts = _one_by_one(cases)
    assert sum(c > cfg[0] for c, (cfg, _, _, _) in zip(counts, cases)) == 31      # more people than max_num_people


def test_match_device_golden_decode_tables(nat, golden_dir):
    assert _one_by_one(_golden_decode_cases(golden_dir)) == [0, 1, 3, 10, 48, 3, 5, 244]


def test_match_device_generated_variants(nat):
    cases = _generated_cases()
    assert len(cases) == 160
    counts = _one_by_one(cases)
    assert all(c > cfg[0] for c, (cfg, _, _, _) in zip(counts, cases)) and max(counts) == 471


def test_match_device_batches_and_compaction(nat, golden_dir):
    """the cases above stacked into batches (one per tag width and parameter set), with images without any candidate
    above the threshold at the start, in the middle and at the end"""
    groups = {}
    for cfg, tag, ind, val in _golden_match_cases(golden_dir) + _golden_decode_cases(golden_dir) + _generated_cases():
        groups.setdefault((cfg, tag.shape[2]), []).append((tag, ind, val))
    largest = 0
    for (cfg, D), items in groups.items():
        empty = (np.zeros((J, K, D), np.float32), np.zeros((J, K), np.int32), np.zeros((J, K), np.float32))
        mid = len(items) // 2
        items = [empty] + items[:mid] + [empty, empty] + items[mid:] + [empty]
        counts = _check_tables(cfg, *(np.stack([it[i] for it in items]) for i in range(3)))
        assert counts[0] == counts[mid + 1] == counts[mid + 2] == counts[-1] == 0
        if len(items) >= 32:
            assert len(set(counts.tolist())) >= 8          # different people counts
        largest = max(largest, len(items))
    assert largest >= 32


def _nudge(x, rng, ulps=3):
    """float32 values moved by a few units in the last place"""
    i = x.astype(np.float32).view(np.int32) + rng.integers(-ulps, ulps + 1, x.shape).astype(np.int32)
    return i.view(np.float32)


def test_match_device_square_root_rounding(nat):
    """the two places a wrongly rounded double square root (or float division) would show: D = 2 with
    use_detection_val=False - the cost IS the distance, one ulp can change an assignment - and D = 1 with tags on a
    half-unit lattice moved by a few ulp, so that many distances sit within a few ulp of tag_threshold = 1 and of a
    half-integer (the rounding of the cost)"""
    rng = np.random.default_rng(1234)
    for trial in range(12):
        val = np.sort(rng.random((J, K)).astype(np.float32), axis=1)[:, ::-1].copy()
        ind = _ind(rng.integers(0, 640, (J, K, 2)))
        tag2 = (rng.integers(0, 5, (J, K, 2)) * 0.75 + rng.normal(0, 0.4, (J, K, 2))).astype(np.float32)
        for cfg in ((30, 0.1, 1.0, False, False), (12, 0.1, 1.0, False, False)):
            _check_tables(cfg, tag2[None], ind[None], val[None])
        lattice = _nudge((rng.integers(0, 14, (J, K, 1)) * 0.5 + 3.0).astype(np.float32), rng)
        lattice[0, :, 0] = (np.arange(K) % 15) * 0.5 + 3.0           # the founders sit on the lattice
        for cfg in (DEFAULT, (30, 0.1, 1.0, False, False), (30, 0.1, 0.5, True, False), (10, 0.1, 1.5, True, False)):
            _check_tables(cfg, lattice[None], ind[None], val[None])
        # several tags per person: the float32 mean and its division (counts of 3, 5, 6, 7 are not powers of two)
        thirds = _nudge((rng.integers(0, 9, (J, K, 1)) / 3.0 + 1.0).astype(np.float32), rng, 1)
        _check_tables((9, 0.1, 1.0, True, False), thirds[None], ind[None], val[None])
        _check_tables((9, 0.1, 1.0, False, False), thirds[None], ind[None], val[None])


def test_match_device_limits_are_errors(nat):
    from rtpe.third_party.group import HeatmapParser
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda:0")  # noqa: E731
    with pytest.raises(RuntimeError, match="at most 64"):
        _parser().match_device(z(1, J, 65, 1), z(1, J, 65, dt=torch.int32), z(1, J, 65), 640)
    with pytest.raises(RuntimeError, match="max_num_people"):
        HeatmapParser(J, 65, 0.1, 1.0, True, False).match_device(z(1, J, K, 1), z(1, J, K, dt=torch.int32), z(1, J, K),
                                                                 640)
    with pytest.raises(RuntimeError, match="at most 32"):
        _parser().match_device(z(1, J, K, 33), z(1, J, K, dt=torch.int32), z(1, J, K), 640)
    nb = ctypes.c_size_t()
    assert nat.lib().rtpe_match_by_tag_dev_scratch_bytes(1, J, 65, 1, ctypes.byref(nb)) < 0
    # the limits themselves work
    rng = np.random.default_rng(5)
    tag = (rng.integers(0, 40, (J, 64, 1)) * 1.5 + rng.normal(0, 0.3, (J, 64, 1))).astype(np.float32)
    val = np.sort(rng.random((J, 64)).astype(np.float32), axis=1)[:, ::-1].copy()
    ind = _ind(rng.integers(0, 640, (J, 64, 2)))
    counts = _check_tables((64, 0.1, 1.0, True, False), tag[None], ind[None], val[None])
    assert counts[0] >= 64


def test_parser_match_method_on_the_device(nat, golden_dir):
    g = np.load(os.path.join(golden_dir, "decode_p30.npz"))
    host, dev = _parser(), _parser(match_on="device")
    want = host.match(g["tag_k"], g["loc_k"], g["val_k"])
    got = dev.match(g["tag_k"], g["loc_k"], g["val_k"])
    assert len(got) == len(want) == 1
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[0], g["matched"])
    e = np.load(os.path.join(golden_dir, "decode_p0.npz"))
    got = dev.match(e["tag_k"], e["loc_k"], e["val_k"])
    assert got[0].shape == (0,) and got[0].dtype == np.float32


# ---- pipeline level: device against host, same inputs, same process -------------------------------------------------
COMBOS = [(True, True), (True, False), (False, True), (False, False)]


def _same_results(got, want, min_people=1):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _assert_same(g, w)
        assert type(g[0]) is type(w[0]) and g[0].dtype == w[0].dtype and g[0].shape == w[0].shape
        assert all(type(s) is np.float32 for s in g[1])
    assert sum(len(w[0]) for w in want) >= min_people


@pytest.mark.parametrize("adjust,refine", COMBOS)
def test_parse_lowres_device_equals_host(nat, adjust, refine):
    P, R, _, _ = _blob_outputs(4, 192, 256, seed=21)
    want = _parser().parse_lowres(R, P[:, J:], (192, 256), adjust, refine)
    got = _parser(match_on="device").parse_lowres(R, P[:, J:], (192, 256), adjust, refine)
    _same_results(got, want, 4)


@pytest.mark.parametrize("adjust,refine", COMBOS)
def test_parse_flip_device_equals_host(nat, adjust, refine):
    outs = _blob_outputs(3, 192, 320, seed=33)
    want = _parser().parse_flip(*outs, adjust=adjust, refine=refine)
    got = _parser(match_on="device").parse_flip(*outs, adjust=adjust, refine=refine)
    _same_results(got, want, 3)
    assert want[0][0].shape[1:] == (J, 5)


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("adjust,refine", COMBOS)
def test_parse_multi_scale_device_equals_host(nat, adjust, refine, flip):
    order = (2, 1, 0.5)
    outs = [o if flip else o[:2] for o in _scale_outputs(3, order, seed=50)]
    want = _parser().parse_multi_scale(outs, (H, W), order, flip, adjust=adjust, refine=refine)
    got = _parser(match_on="device").parse_multi_scale(outs, (H, W), order, flip, adjust=adjust, refine=refine)
    _same_results(got, want, 3)


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("adjust,refine", COMBOS)
def test_parse_multi_scale_ags_device_equals_host(nat, adjust, refine, flip):
    order = (2, 1, 0.5)
    outs = [o if flip else o[:2] for o in _ags_outputs(3, order, seed=31)]
    want = _parser().parse_multi_scale(outs, (H, W), order, flip, adjust=adjust, refine=refine, ags=True)
    got = _parser(match_on="device").parse_multi_scale(outs, (H, W), order, flip, adjust=adjust, refine=refine,
                                                       ags=True)
    _same_results(got, want, 3)
    assert want[0][0].shape[1:] == (J, 4)


def test_images_without_people(nat):
    """a batch in which some images decode to nobody (and one in which all do)"""
    from rtpe.third_party.group import _EMPTY
    P, R, Pf, Rf = _blob_outputs(5, 192, 256, seed=61)
    for t in (R, Rf):
        t[0] = 0
        t[2] = 0
        t[4] = 0
    host, dev = _parser(), _parser(match_on="device")
    for adjust, refine in ((True, True), (False, False)):
        want = host.parse_lowres(R, P[:, J:], (192, 256), adjust, refine)
        got = dev.parse_lowres(R, P[:, J:], (192, 256), adjust, refine)
        _same_results(got, want, 2)
        assert [len(g[0]) > 0 for g in got] == [False, True, False, True, False]
        assert got[0][0].shape == _EMPTY.shape and got[0][1] == []
        _same_results(dev.parse_flip(P, R, Pf, Rf, adjust=adjust, refine=refine),
                      host.parse_flip(P, R, Pf, Rf, adjust=adjust, refine=refine), 2)
    nobody = dev.parse_lowres(torch.zeros_like(R), P[:, J:], (192, 256))
    _same_results(nobody, host.parse_lowres(torch.zeros_like(R), P[:, J:], (192, 256)), 0)
    assert all(p.shape == (0,) and s == [] for p, s in nobody)


def test_noise_maps_at_the_bench_shape(nat, teacher):
    """32 x 640 x 640, W0 weights: noise maps on which every image reaches the 30-people cap"""
    from rtpe.engine import TeacherPipeline
    x = synth.make_images(32, 640, 640).to("cuda:0")
    for kw in (dict(), dict(flip_test=True)):
        want = TeacherPipeline(teacher, _parser(), device="cuda:0", **kw)(x)
        got = TeacherPipeline(teacher, _parser(), device="cuda:0", match_on="device", **kw)(x)
        _same_results(got, want, 32 * 30)
        assert min(len(p) for p, _ in want) >= 30


@pytest.mark.parametrize("flip", [False, True])
def test_stream_on_the_device_equals_call_and_the_host_stream(nat, teacher, flip):
    from rtpe.engine import TeacherPipeline
    dev = TeacherPipeline(teacher, _parser(), device="cuda:0", flip_test=flip, match_on="device")
    host = TeacherPipeline(teacher, _parser(), device="cuda:0", flip_test=flip, match_on="host")
    assert dev.parser.match_on == "device" and host.parser.match_on == "host"
    batches = [synth.make_images(3, 128, 160, seed=70 + k).to("cuda:0") for k in range(5)]
    call = [dev(b) for b in batches]
    got = list(dev.stream(iter(batches)))
    want = list(host.stream(iter(batches)))
    assert len(got) == len(want) == len(call) == 5
    for g, w, c in zip(got, want, call):
        _same_results(g, w, 0)
        _same_results(g, c, 0)
    assert sum(len(p) for r in want for p, _ in r) >= 5
    # None leaves the parser as it is
    p = _parser(match_on="device")
    assert TeacherPipeline(teacher, p, device="cuda:0").parser.match_on == "device"


def test_adjust_refine_n_reads_the_count_on_the_device(nat):
    """rtpe_adjust_refine_fused_topk_n with P_dev at the true count and a capacity far above it: the bits of the plain
    entry called with that count; rows beyond the count are not touched"""
    from rtpe.third_party.group import _match_batch, _ptr
    L = nat.lib()
    P4, R, _, _ = _blob_outputs(3, 192, 256, seed=21)
    tags = P4[:, J:].contiguous()
    parser = _parser()
    st = parser.lowres_topk(R, tags, (192, 256))
    torch.cuda.synchronize()
    h_tag, h_ind, h_val = st["h"]
    flat, pimg, counts = _match_batch(h_tag.numpy(), h_ind.numpy(), h_val.numpy(), 256, parser.params)
    n = flat.shape[0]
    assert n >= 3
    cap = 5 * n + 100
    dev = R.device
    ans_in = torch.full((cap, J, 4), 7.0, device=dev)
    ans_in[:n] = torch.from_numpy(flat).to(dev)
    pimg_d = torch.full((cap,), 1 << 20, dtype=torch.int32, device=dev)      # beyond the count: never an image index
    pimg_d[:n] = torch.from_numpy(pimg).to(dev)
    count = torch.tensor([n], dtype=torch.int32, device=dev)
    h2, w2, h4, w4, hm_stride, tg_stride = st["dims"]
    val_d, ind_d = h_val.to(dev), h_ind.to(dev)
    nb = ctypes.c_size_t()

    def run(entry, P, *extra):
        out = torch.full((cap, J, 4), -5.0, device=dev)
        sc = torch.full((cap,), -5.0, device=dev)
        nat.check(L.rtpe_adjust_refine_scratch_bytes(P, J, 1, ctypes.byref(nb)))
        scr = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        nat.check(entry(_ptr(R), h2, w2, hm_stride, _ptr(tags), h4, w4, tg_stride, 3, J, 192, 256, _ptr(ans_in),
                        _ptr(out), _ptr(pimg_d), P, 1, 1, _ptr(sc), _ptr(val_d), _ptr(ind_d), K, _ptr(scr),
                        scr.numel(), nat.stream_ptr(dev), *extra))
        torch.cuda.synchronize()
        return out.cpu().numpy(), sc.cpu().numpy()
    want, want_sc = run(L.rtpe_adjust_refine_fused_topk, n)
    got, got_sc = run(L.rtpe_adjust_refine_fused_topk_n, cap, _ptr(count))
    assert np.array_equal(got, want) and np.array_equal(got_sc, want_sc)
    assert (got[n:] == -5.0).all() and (got_sc[n:] == -5.0).all()
    assert not np.array_equal(want[:n], flat)                # adjust + refine did something
    assert L.rtpe_adjust_refine_fused_topk_n(_ptr(R), h2, w2, hm_stride, _ptr(tags), h4, w4, tg_stride, 3, J, 192, 256,
                                             _ptr(ans_in), _ptr(ans_in), _ptr(pimg_d), cap, 1, 1, None, _ptr(val_d),
                                             _ptr(ind_d), K, None, 0, None, None) < 0
