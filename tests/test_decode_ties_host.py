"""The stable top-k of the oracle (``HeatmapParserRef(stable_topk=True)``: descending value, ascending flat index - the
order the HIP decode declares among equal values) tied to the reference's ``torch.topk``, on the CPU:

* where no two candidates are equal - every decode golden made by the reference - the two are the same, bit for bit;
* on the tie inputs of oracle/ties.py the VALUES are the same (they are defined even where the order is not) and
  every tie group that fits inside the top K is selected as the same SET of pixels;
* the tie inputs carry the structures the GPU tests (tests/test_decode_ties_gpu.py) rely on, counted on the CPU
  result of the upsampling / aggregation, so that a change to a builder which loses the ties fails here.
"""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import decode_ref, synth, ties


def stable_ref(K=30, ksize=5, pad=2, tag_per_joint=True, stable=True):
    return decode_ref.HeatmapParserRef(17, K, 0.1, 1.0, True, False, tag_per_joint, ksize, pad, stable_topk=stable)


# --------------------------------------------------------------------------- #
# no ties: the stable selection IS torch.topk's
# --------------------------------------------------------------------------- #
def _golden_names(golden_dir):
    return sorted(os.path.basename(p)[len("decode_"):-len(".npz")]
                  for p in glob.glob(os.path.join(golden_dir, "decode_*.npz"))
                  # (decode_dims.npz: the stable oracle reproduces it in tests/test_decode_dims_host.py)
                  if "branches" not in p and "decode_dims" not in p)


def test_every_decode_golden_is_covered(golden_dir):
    assert _golden_names(golden_dir) == sorted(["p0", "p1", "p3", "p10", "p30", "p40", "p3_480", "p5_d2", "lowres_p4",
                                                "lowres_p2_nonsq"])


@pytest.mark.parametrize("name", ["p0", "p1", "p3", "p10", "p30", "p40", "p3_480", "p5_d2", "lowres_p4", "lowres_p2_nonsq"])
def test_stable_oracle_reproduces_the_reference_goldens(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "decode_%s.npz" % name))
    if name.startswith("lowres"):
        P, H, W, oh, ow, seed = [int(v) for v in g["meta"]]
        refined, tags = synth.make_lowres_maps(P, H, W, seed=seed)
        det_t, tag_t = ties.upsampled(torch.from_numpy(refined), torch.from_numpy(tags), (oh, ow))
    else:
        P, h, w, seed, D = [int(v) for v in g["meta"]]
        det, tag = synth.make_decode_maps(P, h, w, seed=seed, tag_dim=D)
        det_t, tag_t = torch.from_numpy(det), torch.from_numpy(tag)
    hp = stable_ref()
    tk = hp.top_k(det_t, tag_t)
    np.testing.assert_array_equal(tk["val_k"], g["val_k"])
    live = g["val_k"] > 0.1                              # the rows that reach match_by_tag; the rest is zero padding,
    assert (g["val_k"][~live] <= 0.1).all()              # whose order ATen does not define
    np.testing.assert_array_equal(tk["loc_k"][live], g["loc_k"][live])
    np.testing.assert_array_equal(tk["tag_k"][live], g["tag_k"][live])
    if "matched" in g.files:
        matched = hp.match(**tk)
        np.testing.assert_array_equal(matched[0], g["matched"])
        adjusted = hp.adjust([m.copy() for m in matched], det_t.numpy())
        np.testing.assert_array_equal(adjusted[0], g["adjusted"])
    ans, scores = hp.parse(det_t, tag_t, adjust=True, refine=True)
    np.testing.assert_array_equal(ans[0], g["final"])
    np.testing.assert_array_equal(np.array(scores, np.float32), g["scores"])


# --------------------------------------------------------------------------- #
# the tie inputs: name -> (hms (1,J,h,w), aes, parser settings, what they must hold)
# --------------------------------------------------------------------------- #
SIZES = [(95, 159), (48, 80), (70, 100), (95, 159)]      # per-image decode sizes of ties.sizes_inputs(): 2 * in - 1,
#                                                          identity (small-output kernel: 48 + 80 <= 128), neither


def _designed(K, D=1, ksize=5, pad=2):
    det, tag = ties.direct_inputs(K, D=D)
    return dict(hms=det, aes=tag, K=K, ksize=ksize, pad=pad, kind="designed")


def _lowres(K, scaled, ksize=5, pad=2):
    refined, tags = ties.lowres_inputs(K)
    hms, aes = ties.upsampled(refined, tags, (319, 447) if scaled else ties.DIRECT_HW)
    return dict(hms=hms, aes=aes, K=K, ksize=ksize, pad=pad, kind="designed", scaled=scaled)


def _sizes(n):
    refined, tags = ties.sizes_inputs()
    hms, aes = ties.upsampled(refined[n:n + 1], tags[n:n + 1], SIZES[n])
    return dict(hms=hms, aes=aes, K=30, kind="lattice" if n != 2 else "generic")


def _net(scales, flip, ags):
    outs = ties.net_outputs(2, scales, seed=3)
    hms, aes = ties.net_maps(outs, scales, flip, 1, ags)
    return dict(hms=hms, aes=aes, K=30, kind="net", tag_per_joint=not ags)


def _big(K):
    det, tag = ties.big_map()
    return dict(hms=det, aes=tag, K=K, kind="big", J=3)


TIE_CASES = {
    "designed_k1": lambda: _designed(1), "designed_k30": lambda: _designed(30), "designed_k64": lambda: _designed(64),
    "designed_k30_d2": lambda: _designed(30, D=2), "designed_k30_3x3": lambda: _designed(30, ksize=3, pad=1),
    "designed_k30_9x9": lambda: _designed(30, ksize=9, pad=4),
    "lowres_identity_k30": lambda: _lowres(30, False), "lowres_scaled_k30": lambda: _lowres(30, True),
    "lowres_scaled_k64": lambda: _lowres(64, True), "lowres_identity_k1": lambda: _lowres(1, False),
    "lowres_scaled_k30_3x3": lambda: _lowres(30, True, 3, 1), "lowres_identity_k30_9x9": lambda: _lowres(30, False, 9, 4),
    "sizes_0": lambda: _sizes(0), "sizes_1": lambda: _sizes(1), "sizes_2": lambda: _sizes(2),
    "sizes_3": lambda: _sizes(3),
    "flip": lambda: _net((1,), True, False), "ms3_flip": lambda: _net((2, 1, 0.5), True, False),
    "ms3": lambda: _net((2, 1, 0.5), False, False), "ms1": lambda: _net((1,), False, False),
    "ms3_flip_ags": lambda: _net((2, 1, 0.5), True, True), "ms1_ags": lambda: _net((1,), False, True),
    "ms3_ags": lambda: _net((2, 1, 0.5), False, True), "ms1_flip_ags": lambda: _net((1,), True, True),
    "big_k8": lambda: _big(8), "big_k30": lambda: _big(30),
}


def case_ref(c, stable=True):
    ref = stable_ref(c["K"], c.get("ksize", 5), c.get("pad", 2), c.get("tag_per_joint", True), stable)
    ref.params.num_joints = c.get("J", 17)
    return ref


def check_structure(c):
    """the structures the case is there for, counted on the oracle's result; returns the counts"""
    ref = case_ref(c)
    if c["kind"] == "big":
        # d: more tiles than the head merge keeps in registers; a tie group at the K-th place, tie groups inside,
        # zero padding behind a tie group, a plateau around a tile corner
        K = c["K"]
        nms = ref.nms(c["hms"])[0].numpy()
        s = [ties.topk_structure(p, K) for p in nms]
        assert s[0]["tiles"] == 2209 > 2048
        assert s[0]["straddle"] is not None and s[0]["straddle"][3] and s[0]["other_tile_row"] >= 1, s[0]["straddle"]
        assert s[1]["positives"] == 5 and (len(s[1]["padding"]) == K - 5 if K > 5 else True) and (0.5, 5) in s[1]["groups"]
        assert s[2]["corner4"] == 1 and s[2]["straddle"] is not None and s[2]["straddle"][3]
        keys_kib = s[0]["tiles"] * K * 8 / 1024.0
        assert keys_kib > 150 if K == 30 else keys_kib + 32 / 1024.0 <= 150           # global scan / LDS scan
        return dict(tiles=s[0]["tiles"], key_list_kib=keys_kib, straddle=[p["straddle"] for p in s])
    s = ties.summarize(ref, c["hms"], c["aes"])
    if c["kind"] == "designed":
        return ties.require_designed(s, c.get("scaled", False))
    if c["kind"] == "generic":       # a size that is neither the identity nor 2 * in - 1: the upsampling is inexact and
        assert s["groups"] >= 1      # promises no structure; the image makes the batch heterogeneous, yet ties survive
        return dict(groups=s["groups"])
    return ties.require_lattice(s, plateau_tile=c["kind"] == "net")


@pytest.mark.parametrize("name", sorted(TIE_CASES))
def test_tie_inputs_hold_their_structures(name):
    print(name, check_structure(TIE_CASES[name]()))


@pytest.mark.parametrize("name", sorted(TIE_CASES))
def test_stable_and_torch_topk_agree_where_the_reference_is_defined(name):
    c = TIE_CASES[name]()
    a = case_ref(c).top_k(c["hms"], c["aes"])
    b = case_ref(c, stable=False).top_k(c["hms"], c["aes"])
    np.testing.assert_array_equal(a["val_k"], b["val_k"])
    nms = case_ref(c).nms(c["hms"])[0].numpy()
    w = nms.shape[2]
    whole, cut = 0, 0
    for j, plane in enumerate(nms):
        ia = a["loc_k"][0, j, :, 1] * w + a["loc_k"][0, j, :, 0]
        ib = b["loc_k"][0, j, :, 1] * w + b["loc_k"][0, j, :, 0]
        assert np.array_equal(plane.reshape(-1)[ia], a["val_k"][0, j]) and len(set(ia.tolist())) == len(ia)
        for v in np.unique(a["val_k"][0, j]):
            mine = a["val_k"][0, j] == v
            if int((plane == v).sum()) == int(mine.sum()):          # the whole tie group fits: the same pixels
                assert set(ia[mine].tolist()) == set(ib[b["val_k"][0, j] == v].tolist()), (j, v)
                whole += int(mine.sum()) > 1
            else:
                assert np.array_equal(ia[mine], np.flatnonzero(plane.reshape(-1) == v)[:int(mine.sum())]), (j, v)
                cut += 1
    assert whole >= 1 or c["K"] == 1 or c["kind"] == "generic"
    assert cut >= 1
