"""The decode at every tag dimension and on the rare branches of refine, CPU side (oracle/tagdims.py):

* the oracle reproduces tests/golden/decode_dims.npz - the reference's own HeatmapParser / match_by_tag, run with the
  real munkres package on the same seeded scenes (tools/gen_golden.py --only decode_dims) - bit for bit;
* every scene has the structure it exists for (``*_structure`` counts on the oracle's result);
* seeded faults: the oracle asked for a wrong float order, the mean from the rows' columns, the first 512 people only,
  a slot mix-up, or D == 1 without the exact expression changes the rows of the scene made for it - and leaves the
  blob scenes as they are, which is why blobs were not enough;
* ``pairwise8_sum_f32`` against ``np.add.reduce`` for every length the kernels can meet.

The GPU side is tests/test_decode_dims_gpu.py; the helpers here are shared with it."""
import os

import numpy as np
import pytest

from oracle import decode_ref
from oracle import tagdims as T

BLOBS = {c["name"]: c for c in T.blob_cases()}
MATCH = {c[0]: c for c in T.match_cases()}
_CACHE = {}


def cached(key, make):
    """reference results are computed once per process and shared, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = T.unpack_results(np.load(os.path.join(golden_dir, "decode_dims.npz")))
    assert int(g["real_package"]) == 1, "the fixture must come from the real munkres package"
    assert tuple(g["dims"]) == T.DIMS
    return g


def same_digest(a, want, what):
    assert np.array_equal(T.digest(np.asarray(a, np.float32)), want), what


def blob_oracle(name):
    """the oracle's stages on a blob case: top-k, matched, adjusted, and parse under the four switches"""
    def make():
        c = BLOBS[name]
        det, tag = T.blob_maps(c)
        hp = T.blob_parser(c)
        tk = hp.top_k(det, tag)
        matched = hp.match(**tk)
        adjusted = hp.adjust([m.copy() for m in matched], det.numpy())
        parsed = {(a, r): hp.parse(det, tag, a, r) for a in (True, False) for r in (True, False)}
        return dict(det=det, tag=tag, tk=tk, matched=matched[0], adjusted=adjusted[0], parsed=parsed)
    return cached(("blob", name), make)


def boundary(D):
    return cached(("b", D), lambda: T.boundary_scene(D))


def people(name):
    return cached(("c", name), lambda: T.people_case(name))


def refined(key, scene, **kw):
    return cached(("refined", key, tuple(sorted(kw.items()))), lambda: T.refine_rows(scene, **kw))


# --------------------------------------------------------------------------- #
# the oracle against the reference's recorded results
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", sorted(BLOBS))
def test_blobs_match_the_reference(golden, name):
    c, o, k = BLOBS[name], blob_oracle(name), "a_" + name
    assert tuple(golden[k + "_meta"]) == (c["persons"], c["h"], c["w"], c["seed"], c["D"], int(c["tag_per_joint"]))
    tk = o["tk"]
    same_digest(tk["val_k"], golden[k + "_val_k"], "val_k")
    live = tk["val_k"] > 0.1
    assert np.array_equal(np.packbits(live), golden[k + "_live"])
    np.testing.assert_array_equal(tk["loc_k"][live], golden[k + "_loc_k"])
    same_digest(tk["tag_k"][live], golden[k + "_tag_k"], "tag_k")
    same_digest(o["matched"], golden[k + "_matched"], "matched")
    same_digest(o["adjusted"], golden[k + "_adjusted"], "adjusted")
    ans, scores = o["parsed"][True, True]
    np.testing.assert_array_equal(ans[0][:, :, :3], golden[k + "_final_xyv"])
    same_digest(ans[0], golden[k + "_final"], "final")
    np.testing.assert_array_equal(np.array(scores, np.float32), golden[k + "_scores"])
    # no ties on these maps: the stable selection the HIP decode declares is torch.topk's
    stable = T.blob_parser(c, stable_topk=True)
    tk_s = stable.top_k(o["det"], o["tag"])
    for key in ("val_k", "loc_k", "tag_k"):
        np.testing.assert_array_equal(tk_s[key], tk[key], err_msg=key)
    same_digest(stable.parse(o["det"], o["tag"])[0][0], golden[k + "_final"], "final, stable top-k")
    st = T.blob_structure(c, tk, o["adjusted"], ans[0])
    print(name, st)
    # what a blob case is for: candidates with D-wide tags, all its people, and joints left for refine's D-wide scan
    assert st["tag_dim"] == c["D"] and st["people"] >= c["persons"] and st["filled"] >= 1 and st["live"] >= 17


@pytest.mark.parametrize("D", T.BOUNDARY_DIMS)
def test_boundary_and_foreign_rows_match_the_reference(golden, D):
    s = boundary(D)
    rows = refined(("b", D), s)
    np.testing.assert_array_equal(rows[:, :, :3], golden["b_d%d_xyv" % D])
    same_digest(rows, golden["b_d%d" % D], "refined rows")
    for kind in T.FOREIGN:
        f = T.foreign_rows(s, kind)
        rows_f = T.refine_rows(f)
        np.testing.assert_array_equal(rows_f[:, :, :3], golden["e_d%d_%s_xyv" % (D, kind)], err_msg=kind)
        same_digest(rows_f, golden["e_d%d_%s" % (D, kind)], kind)
        # the reference reads the map: the answers are those of the consistent rows, the columns the caller's
        np.testing.assert_array_equal(rows_f[:, :, :3], rows[:, :, :3])
        np.testing.assert_array_equal(rows_f[:, :, 3:], f["rows"][:, :, 3:])


@pytest.mark.parametrize("name", sorted(T.PEOPLE_SCENES))
def test_people_match_the_reference(golden, name):
    rows = refined(("c", name), people(name))
    want = golden["c_" + name + "_xyv"]
    np.testing.assert_array_equal(rows[-40:, :, :3] if len(rows) > 64 else rows[:, :, :3], want)
    same_digest(rows, golden["c_" + name], name)


def test_overflow_matches_the_reference(golden):
    rows = T.refine_rows(T.overflow_scene())
    np.testing.assert_array_equal(rows[:, :, :3], golden["d_xyv"])
    same_digest(rows, golden["d"], "overflow")


def test_matcher_tables_match_the_reference(golden):
    assert len(MATCH) == 4 * len(T.DIMS) + 2 * sum(D >= 8 for D in T.DIMS)
    for name, (_, cfg, tag, loc, val) in MATCH.items():
        ans = decode_ref.match_by_tag(tag, loc, val, T.match_params(cfg))
        assert tuple(golden["f_" + name + "_shape"]) == ans.shape, name
        same_digest(ans, golden["f_" + name], name)


def test_host_matcher_on_the_tables():
    """csrc/match_host.cpp (CPU code of the extension) on the same tables: the people of the oracle, bit for bit"""
    import __graft_entry__ as g
    g.build()
    from rtpe.third_party.group import _W_ENC, HeatmapParser, _match_batch
    for name, (_, cfg, tag, loc, val) in MATCH.items():
        ind = (loc[..., 1] * _W_ENC + loc[..., 0]).astype(np.int32)
        par = HeatmapParser(T.F_J, *cfg)
        flat, _, counts = _match_batch(tag[None], ind[None], val[None], _W_ENC, par.params)
        want = decode_ref.match_by_tag(tag, loc, val, T.match_params(cfg))
        assert flat.shape == want.shape and np.array_equal(flat.view(np.uint32), want.view(np.uint32)), name


# --------------------------------------------------------------------------- #
# the structures
# --------------------------------------------------------------------------- #
def check_boundary(D):
    st = cached(("b_structure", D), lambda: T.boundary_structure(boundary(D)))
    for fault in T.ORDER_FAULTS:
        for direction in (1, 2):
            n = st["pairs"][fault, direction]
            if T.fault_applies(fault, D) and not (fault == "no_tail" and direction == 1):
                assert n >= 1, (D, fault, direction, st)
            else:
                assert n == 0, (D, fault, direction, st)
        assert st["at_maximum"][fault] >= int(T.fault_applies(fault, D)), (D, fault, st)
    assert st["filled"] == 18                              # both people, the nine missing planes
    return st


def check_people(name):
    s = people(name)
    st = cached(("c_structure", name), lambda: T.people_structure(s))
    counts, D, J, found = T.PEOPLE_SCENES[name]
    assert s["tag"].shape[4] == D and s["det"].shape[1] == J
    if name.startswith("c40"):
        assert st["missing"] == [40] and st["passes"] == [3] and st["filled"] == 40
        assert len({tuple(r[3, :3]) for r in refined(("c", name), s)}) == 40          # distinct answers
    elif name.startswith("c530"):
        assert st["missing"] == [530] and st["trips"] == [2] and st["beyond_unique"] == 18 and st["filled"] == 530
    elif name.startswith("c3img"):
        assert st["missing"] == [200, 0, 330] and st["passes"] == [13, 0, 21] and st["filled"] == 530
    elif name == "j32_d32":
        assert (J, D) == (32, 32) and st["filled"] == 3 * 16
    else:
        assert J == 1 and st["filled"] == 0
    return st


@pytest.mark.parametrize("D", T.BOUNDARY_DIMS)
def test_boundary_structure(D):
    print(D, check_boundary(D))


@pytest.mark.parametrize("name", sorted(T.PEOPLE_SCENES))
def test_people_structure(name):
    print(name, check_people(name))


def check_overflow():
    st = T.overflow_structure(T.overflow_scene())
    assert st["overflowed"] == st["pixels"] == 240 and st["magnitudes"] >= 3
    assert st["finite_heat"] and st["pixel0"] and st["fast_differs"] and st["no_nan"]
    return st


def test_overflow_structure():
    print(check_overflow())


def check_match_structure():
    n = {name: T.match_structure(c) for name, c in MATCH.items()}
    assert all(v == 0 for k, v in n.items() if k.startswith("rand"))
    assert sum(v for k, v in n.items() if k.startswith("dist")) == 5
    assert sum(v for k, v in n.items() if k.startswith("centre")) == 5
    return n


def test_match_structure():
    check_match_structure()


def check_wide():
    def make():
        hms, aes = T.wide_maps()
        hp = decode_ref.HeatmapParserRef()
        tk = hp.top_k(hms, aes)
        adjusted = hp.adjust([m.copy() for m in hp.match(**tk)], hms.numpy())[0]
        st = T.wide_structure(hms, aes, adjusted)
        assert st["width"] > T.ARGMAX_WIDTH and st["people"] == 3 and st["shortcut"] >= 1 and st["scan"] >= 1, st
        return dict(hms=hms, aes=aes, st=st,
                    parsed={(a, r): hp.parse(hms, aes, a, r) for a in (True, False) for r in (True, False)})
    return cached("wide", make)


def test_wide_structure():
    print(check_wide()["st"])


# --------------------------------------------------------------------------- #
# seeded faults
# --------------------------------------------------------------------------- #
def _blob_scene(name):
    o, c = blob_oracle(name), BLOBS[name]
    tag = o["tag"][0].numpy()
    if not c["tag_per_joint"]:
        tag = np.tile(tag, (17, 1, 1, 1))
    return dict(det=o["det"].numpy(), tag=tag[None], rows=o["adjusted"], pimg=np.zeros(len(o["adjusted"]), np.int32))


@pytest.mark.parametrize("fault", decode_ref.FAULTS + T.BATCH_FAULTS)
def test_seeded_fault_leaves_the_blobs_unchanged(fault):
    changed = 0
    for name in sorted(BLOBS):
        s = _blob_scene(name)
        want = blob_oracle(name)["parsed"][True, True][0][0]
        np.testing.assert_array_equal(T.refine_rows(s), want)                 # (the runner is the oracle's parse)
        if fault == "no_tail" and BLOBS[name]["D"] in (9, 17):
            # the one fault that is not subtle: a whole coordinate of a 3-apart tag is gone, and blobs at the D
            # where there is a tail do see it (p4_d9 does); at every other D it is the reference's sum
            changed += not np.array_equal(T.refine_rows(s, fault), want)
            continue
        np.testing.assert_array_equal(T.refine_rows(s, fault), want, err_msg="%s %s" % (fault, name))
        if fault in ("sequential", "pairwise_mean"):
            tk, c = blob_oracle(name)["tk"], BLOBS[name]
            wrong = T.blob_parser(c).match(fault=fault, **tk)[0]
            np.testing.assert_array_equal(wrong, blob_oracle(name)["matched"])
    assert changed >= 1 or fault != "no_tail"


@pytest.mark.parametrize("fault", T.ORDER_FAULTS)
def test_wrong_float_order_changes_the_boundary_scene(fault):
    dims = [D for D in T.BOUNDARY_DIMS if T.fault_applies(fault, D)]
    assert len(dims) >= 2
    for D in dims:
        s = boundary(D)
        assert not np.array_equal(T.refine_rows(s, fault), refined(("b", D), s)), (fault, D)


def test_mean_from_the_rows_columns_changes_the_foreign_rows():
    half = 0
    for D in T.BOUNDARY_DIMS:
        s = boundary(D)
        np.testing.assert_array_equal(T.refine_rows(s, "row_mean"), refined(("b", D), s))   # consistent rows: no change
        for kind in ("zeros", "other"):
            f = T.foreign_rows(s, kind)
            assert not np.array_equal(T.refine_rows(f, "row_mean"), T.refine_rows(f)), (D, kind)
        f = T.foreign_rows(s, "half")
        half += not np.array_equal(T.refine_rows(f, "row_mean"), T.refine_rows(f))
    assert half >= 4


def test_batch_faults_change_the_people_scenes():
    for name in ("c530_d1", "c530_d3"):
        s = people(name)
        right, wrong = refined(("c", name), s), T.refine_rows(s, "first512")
        assert np.array_equal(wrong[:512], right[:512]) and (wrong[512:, 3, 2] == 0).all() and (right[512:, 3, 2] > 0).all()
    for name in ("c40_d1", "c40_d3", "c530_d1", "c530_d3", "c3img_d1", "c3img_d3"):
        s = people(name)
        assert not np.array_equal(T.refine_rows(s, "slot16"), refined(("c", name), s)), name
    for name in ("j32_d32", "j1_d1"):
        s = people(name)
        for fault in T.BATCH_FAULTS:
            np.testing.assert_array_equal(T.refine_rows(s, fault), refined(("c", name), s))


def test_no_exact_fallback_changes_the_overflow_scene():
    s = T.overflow_scene()
    right, fast = T.refine_rows(s), T.refine_rows(s, "no_fallback")
    assert (right[0, 3, 0], right[0, 3, 1]) == (0.25, 0.25) or right[0, 3, 0] < 1
    assert (fast[0, 3, 0], fast[0, 3, 1]) != (right[0, 3, 0], right[0, 3, 1])
    for D in (2, 9):                                        # nothing overflows there: the fast form is the reference's
        b = boundary(D)
        np.testing.assert_array_equal(T.refine_rows(b, "no_fallback"), refined(("b", D), b))
    c = people("c40_d1")
    np.testing.assert_array_equal(T.refine_rows(c, "no_fallback"), refined(("c", "c40_d1"), c))


# --------------------------------------------------------------------------- #
# numpy's pairwise walk at every length
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", range(1, 33))
def test_pairwise8_sum_equals_numpy_at_every_length(n):
    rng = np.random.default_rng(n)
    differs = 0
    for trial in range(200):
        a = (rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
        got, want = decode_ref.pairwise8_sum_f32(a), np.add.reduce(np.ascontiguousarray(a))
        assert got.dtype == np.float32 and got.view(np.int32) == want.view(np.int32), (n, trial)
        s = np.float32(0)
        for v in a:
            s = np.float32(s + v)
        differs += s != want
    assert differs > 0 or n < 8                             # from 8 on the order is visible on this data
