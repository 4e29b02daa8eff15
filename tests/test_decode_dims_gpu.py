"""The HIP decode at every tag dimension D and on the rare branches of refine (scenes and counters: oracle/tagdims.py;
their CPU side, the reference fixture and the seeded faults: tests/test_decode_dims_host.py).

The kernels restate numpy's float orders keyed on D - the mean tag (pairwise for D == 1, sequential otherwise), the
squared distances of refine's shortcut and scan (sequential below 8, ``pairwise8_sum`` with its block loop, tree and
tail from 8 on), the matcher's float64 distances and float32 centres - and the scenes put tags on the rounding boundary
of each, so a kernel that sums in another order, contracts the squares into fmas or drops the tail returns another
pixel.  Further: more than 16 people missing one joint (the static-index slot update), more than 512 people of an image
(the second trip of the scan), an empty image between two full ones, J = 32 with D = 32, squared distances that
overflow (the exact expression of the D == 1 scan), rows with foreign tag columns through ``HeatmapParser.refine``,
and fused maps wider than the 2,048 columns of the plane-maximum pass.

Every test first asserts the structure counts, then compares EVERY element with the oracle - and with the reference's
recorded results where the reference has the path - bit for bit (-0 folded onto +0).  No tolerances."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import decode_ref
from oracle import tagdims as T
from test_decode_dims_host import (BLOBS, MATCH, blob_oracle, boundary, cached, check_boundary, check_match_structure,
                                   check_overflow, check_people, check_wide, golden, people, refined,  # noqa: F401
                                   same_digest)
from test_decode_ties_gpu import _cuda, _same, _same_people

pytestmark = pytest.mark.gpu

SWITCHES = ((True, True), (False, True), (True, False), (False, False))      # (adjust, refine)
PRESET = -5.0                                # what the rows beyond the people hold before and after an "_n" call


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    assert _native.lib().rtpe_device_count() >= 1
    return _native


def _parser(J=17, K=30, match_on="host", cfg=(0.1, 1.0, True, False), tag_per_joint=True):
    from rtpe.third_party.group import HeatmapParser
    return HeatmapParser(J, K, *cfg, tag_per_joint, 5, 2, match_on=match_on)


# --------------------------------------------------------------------------- #
# a. blobs: top_k, match, adjust, parse
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", sorted(BLOBS))
def test_blobs_through_every_stage(nat, golden, name):
    c, o, k = BLOBS[name], blob_oracle(name), "a_" + name
    st = T.blob_structure(c, o["tk"], o["adjusted"], o["parsed"][True, True][0][0])
    assert st["tag_dim"] == c["D"] and st["people"] >= c["persons"] and st["filled"] >= 1 and st["live"] >= 17
    det_d, tag_d = _cuda(o["det"], o["tag"])
    host, dev = (_parser(match_on=m, tag_per_joint=c["tag_per_joint"]) for m in ("host", "device"))
    got = host.top_k(det_d, tag_d)
    for key in ("val_k", "loc_k", "tag_k"):
        _same(got[key], o["tk"][key], (name, key))
    live = got["val_k"] > 0.1
    same_digest(got["val_k"], golden[k + "_val_k"], "val_k")
    _same(got["loc_k"][live], golden[k + "_loc_k"].astype(np.int64), (name, "loc_k, reference"))
    same_digest(got["tag_k"][live], golden[k + "_tag_k"], "tag_k")
    for par in (host, dev):
        m = par.match(**got)
        assert len(m) == 1
        _same(m[0], o["matched"], (name, par.match_on, "matched"))
        same_digest(m[0], golden[k + "_matched"], "matched")
    adjusted = host.adjust([o["matched"].copy()], det_d)[0]
    _same(adjusted, o["adjusted"], (name, "adjusted"))
    same_digest(adjusted, golden[k + "_adjusted"], "adjusted")
    for a, r in SWITCHES:
        ans, scores = host.parse(det_d, tag_d, adjust=a, refine=r)
        want = o["parsed"][a, r]
        _same_people((ans[0], scores), (want[0][0], want[1]), (name, a, r))
    ans, scores = host.parse(det_d, tag_d)
    same_digest(ans[0], golden[k + "_final"], "final")
    _same(np.array(scores, np.float32), golden[k + "_scores"], (name, "scores, reference"))


@pytest.mark.parametrize("D", [1, 3])
def test_parse_with_one_joint(nat, D):
    """J = 1: every candidate founds a person, nothing is left to refine"""
    from oracle import synth
    det, tag = synth.make_decode_maps(5, 40, 72, 77, sigma=1.5, tag_dim=D, joints=1, drop=0.0)
    det, tag = torch.from_numpy(det), torch.from_numpy(tag)
    ref, par = decode_ref.HeatmapParserRef(num_joints=1), _parser(J=1)
    det_d, tag_d = _cuda(det, tag)
    for a, r in SWITCHES:
        want = ref.parse(det, tag, a, r)
        assert len(want[0][0]) == 5
        ans, scores = par.parse(det_d, tag_d, adjust=a, refine=r)
        _same_people((ans[0], scores), (want[0][0], want[1]), (D, a, r))


# --------------------------------------------------------------------------- #
# b, c, d. refine through rtpe_adjust_refine, and through the entry that reads the number of people on the device
# --------------------------------------------------------------------------- #
def _scene(kind, key):
    if kind == "b":
        check_boundary(key)
        return boundary(key)
    if kind == "c":
        check_people(key)
        return people(key)
    check_overflow()
    return cached("d", T.overflow_scene)


def _scores(rows):
    return np.array([decode_ref.pairwise8_sum_f32(np.ascontiguousarray(r[:, 2])) / np.float32(len(r)) for r in rows],
                    np.float32)


REFINE_SCENES = [("b", D) for D in T.BOUNDARY_DIMS] + [("c", n) for n in sorted(T.PEOPLE_SCENES)] + [("d", 0)]


@pytest.mark.parametrize("kind,key", REFINE_SCENES, ids=["%s_%s" % s for s in REFINE_SCENES])
def test_refine_scenes(nat, golden, kind, key):
    s = _scene(kind, key)
    det_d, tag_d = _cuda(torch.from_numpy(s["det"]), torch.from_numpy(s["tag"]))
    par = _parser(J=s["det"].shape[1])
    for adj in (False, True):
        want = refined((kind, key), s, do_adjust=adj) if adj else refined((kind, key), s)
        got, sc = par._adjust_refine(det_d, tag_d, s["rows"], s["pimg"], adj, True)
        _same(got, want, (kind, key, adj))
        _same(sc, _scores(s["rows"]), (kind, key, adj, "scores"))
        if not adj:
            same_digest(got, golden[{"b": "b_d%s" % key, "c": "c_%s" % key, "d": "d"}[kind]], (kind, key))
    only_adjust, _ = par._adjust_refine(det_d, tag_d, s["rows"], s["pimg"], True, False)
    _same(only_adjust, T.refine_rows(s, do_adjust=True, do_refine=False), (kind, key, "adjust only"))


N_SCENES = [("c", n) for n in sorted(T.PEOPLE_SCENES) if T.PEOPLE_SCENES[n][1] == 1] + [("d", 0)]


@pytest.mark.parametrize("kind,key", N_SCENES, ids=["%s_%s" % s for s in N_SCENES])
def test_refine_scenes_with_the_count_on_the_device(nat, kind, key):
    """``rtpe_adjust_refine_fused_topk_n`` on the D == 1 scenes (the fused entries take one tag per pixel), the maps
    decoded at their own size: the buffers hold 37 rows more than there are people, and those stay as preset"""
    from rtpe.third_party.group import _ptr
    s = _scene(kind, key)
    N, J, h, w = s["det"].shape
    P = len(s["rows"])
    cap = P + 37
    det_d, tag_d = _cuda(torch.from_numpy(s["det"]), torch.from_numpy(np.ascontiguousarray(s["tag"][..., 0])))
    par = _parser(J=J)
    st = par.lowres_topk(det_d, tag_d, (h, w))
    entry, head, takes_topk = st["refine"]
    assert takes_topk and entry == "rtpe_adjust_refine_fused_topk"
    _, h_ind, h_val = st["h"]
    L = nat.lib()
    nb = ctypes.c_size_t()
    nat.check(L.rtpe_adjust_refine_scratch_bytes(cap, J, 1, ctypes.byref(nb)))
    for adj in (False, True):
        ans_in = torch.full((cap, J, 4), 7.0, device="cuda:0")          # rows beyond the people: never to be read
        ans_in[:P] = torch.from_numpy(s["rows"]).to("cuda:0")
        pimg = torch.full((cap,), N - 1, dtype=torch.int32, device="cuda:0")
        pimg[:P] = torch.from_numpy(s["pimg"]).to("cuda:0")
        out = torch.full((cap, J, 4), PRESET, device="cuda:0")
        sc = torch.full((cap,), PRESET, device="cuda:0")
        total = torch.tensor([P], dtype=torch.int32, device="cuda:0")
        scratch = torch.empty(nb.value, dtype=torch.uint8, device="cuda:0")
        nat.check(getattr(L, entry + "_n")(*head, _ptr(ans_in), _ptr(out), _ptr(pimg), cap, int(adj), 1, _ptr(sc),
                                           _ptr(h_val), _ptr(h_ind), h_val.shape[2], _ptr(scratch), scratch.numel(),
                                           nat.stream_ptr(det_d.device), _ptr(total)))
        torch.cuda.synchronize()
        want = refined((kind, key), s, do_adjust=adj) if adj else refined((kind, key), s)
        _same(out[:P].cpu().numpy(), want, (kind, key, adj))
        _same(sc[:P].cpu().numpy(), _scores(s["rows"]), (kind, key, adj, "scores"))
        assert bool((out[P:] == PRESET).all()) and bool((sc[P:] == PRESET).all())


# --------------------------------------------------------------------------- #
# e. HeatmapParser.refine with foreign tag columns
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("D", T.BOUNDARY_DIMS)
def test_refine_reads_the_map_not_the_rows(nat, golden, D):
    check_boundary(D)
    s = boundary(D)
    par = _parser()
    det_d, tag_d = _cuda(torch.from_numpy(s["det"][0]), torch.from_numpy(s["tag"][0]))
    consistent = refined(("b", D), s)
    for kind in T.FOREIGN:
        f = T.foreign_rows(s, kind)
        assert not np.array_equal(f["rows"][:, :, 3:], s["rows"][:, :, 3:])
        got = np.stack([par.refine(det_d, tag_d, f["rows"][p].copy()) for p in range(2)])
        _same(got, T.refine_rows(f), (D, kind))
        _same(got[:, :, :3], consistent[:, :, :3], (D, kind, "the answers of the consistent rows"))
        _same(got[:, :, 3:], f["rows"][:, :, 3:], (D, kind, "the caller's columns"))
        same_digest(got, golden["e_d%d_%s" % (D, kind)], (D, kind))


# --------------------------------------------------------------------------- #
# f. matcher tables
# --------------------------------------------------------------------------- #
def _ind(loc):
    from rtpe.third_party.group import _W_ENC
    return (loc[..., 1].astype(np.int64) * _W_ENC + loc[..., 0].astype(np.int64)).astype(np.int32)


def _match_both(cfg, tag, ind, val):
    """tag (N,J,K,D), ind (N,J,K), val (N,J,K) through the host matcher and the grouping kernel -> the host's
    (flat, counts), after the kernel's four outputs were compared with it bit for bit"""
    from rtpe.third_party.group import _W_ENC, _match_batch
    par = _parser(K=cfg[0], cfg=cfg[1:])
    flat, pimg, counts = _match_batch(tag, ind, val, _W_ENC, par.params)
    ans, pimg_d, counts_d, total = par.match_device(torch.from_numpy(np.ascontiguousarray(tag, np.float32)),
                                                    torch.from_numpy(np.ascontiguousarray(ind, np.int32)),
                                                    torch.from_numpy(np.ascontiguousarray(val, np.float32)), _W_ENC)
    n = int(total.cpu()[0])
    assert n == flat.shape[0] == int(counts.sum()) and np.array_equal(counts_d.cpu().numpy(), counts)
    assert np.array_equal(pimg_d[:n].cpu().numpy(), pimg)
    got = ans[:n].cpu().numpy()
    assert got.shape == flat.shape and np.array_equal(got.view(np.uint32), flat.view(np.uint32))
    return flat, counts


def _match_oracle(name):
    _, cfg, tag, loc, val = MATCH[name]
    return cached(("f", name), lambda: decode_ref.match_by_tag(tag, loc, val, T.match_params(cfg)))


@pytest.mark.parametrize("D", T.DIMS)
def test_matcher_tables(nat, golden, D):
    counts = check_match_structure()
    names = [n for n in MATCH if n.endswith("_d%d" % D) or "_d%d_" % D in n]
    assert len(names) == 4 + 2 * (D >= 8) and sum(counts[n] for n in names) == 2 * (D >= 8)
    groups = {}
    for name in names:
        _, cfg, tag, loc, val = MATCH[name]
        want = _match_oracle(name)
        flat, _ = _match_both(cfg, tag[None], _ind(loc)[None], val[None])
        _same(flat, want.reshape(flat.shape) if want.size == 0 else want, (name, "one by one"))
        same_digest(want, golden["f_" + name], name)
        groups.setdefault(cfg, []).append((name, tag, _ind(loc), val))
    for cfg, items in groups.items():                       # one batch per parameter set, empty images between
        empty = ("", np.zeros((T.F_J, T.F_K, D), np.float32), np.zeros((T.F_J, T.F_K), np.int32),
                 np.zeros((T.F_J, T.F_K), np.float32))
        mid = (len(items) + 1) // 2
        batch = [empty] + items[:mid] + [empty, empty] + items[mid:] + [empty]
        flat, counts = _match_both(cfg, *(np.stack([it[i] for it in batch]) for i in (1, 2, 3)))
        at = 0
        for (name, _, _, _), c in zip(batch, counts):
            if name:
                _same(flat[at:at + c], _match_oracle(name), (name, "in the batch"))
            else:
                assert c == 0
            at += int(c)


# --------------------------------------------------------------------------- #
# g. fused maps wider than 2,048 pixels
# --------------------------------------------------------------------------- #
def _wide(par, adjust=True, refine=True):
    w = check_wide()
    assert w["st"]["width"] > T.ARGMAX_WIDTH and w["st"]["shortcut"] >= 1 and w["st"]["scan"] >= 1
    res = par.parse_lowres(*_cuda(*T.wide_inputs()), T.WIDE_HW, adjust=adjust, refine=refine)
    assert len(res) == 1
    want = w["parsed"][adjust, refine]
    _same_people(res[0], (want[0][0], want[1]), ("wide", par.match_on, adjust, refine))


@pytest.mark.parametrize("match_on", ["host", "device"])
def test_parse_lowres_wider_than_2048(nat, match_on):
    for a, r in SWITCHES:
        _wide(_parser(match_on=match_on), a, r)


def test_parse_lowres_wider_than_2048_with_the_plane_maximum_pass(nat, monkeypatch):
    """RTPE_REFINE_TOPK=0: refine's plane maxima come from ``plane_argmax_kernel``, which walks a map of more than
    256 * 8 columns pixel by pixel instead of by owned columns"""
    monkeypatch.setenv("RTPE_REFINE_TOPK", "0")
    _wide(_parser())
