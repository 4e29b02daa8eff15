"""GPU tests of the keypoint scoring: the kernel's OKS matrix, match tables and result rows against the float64
restatement (tests/scoring_restated.py) on the seeded set and the hand cases of tests/test_scoring_host.py, the ten
statistics of ``score_records``, and the path from a ``StudentPipeline`` to the reference's dict."""
import numpy as np
import pytest
import torch

import scoring_restated as SR
import test_scoring_host as H
from test_student_pipeline_gpu import _det, _parser

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = SR.MAX_DETS
# |kernel OKS - restatement OKS| ("Scoring"): both sum the same <= 17 terms exp(-e) <= 1 in the same
# order and divide by the same count; the terms differ by the two exps' errors, at most EXP_ULPS_DEVICE + EXP_ULPS_NUMPY
# units of 2^-52 (documented: 1 ulp for the device library's double exp, below 1 ulp for the host libm's); n - 1 additions
# with partial sums below 32 round by at most 2^-49 on either side, i.e. 2^-48 after the division by n; the two divisions
# round by 2^-54 each
EXP_ULPS_DEVICE, EXP_ULPS_NUMPY = 1, 1
OKS_BOUND = (EXP_ULPS_DEVICE + EXP_ULPS_NUMPY) * 2.0 ** -52 + 2.0 ** -48 + 2.0 ** -53


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    return _native


def _records(dt):
    from rtpe import engine
    ids = list(dt)
    return engine.pack_records(ids, [dt[i] for i in ids], DEV)


def _sets():
    """name -> (dt, gt, ids): the seeded set and the hand cases"""
    sets = {"seeded": H.seeded_set()}
    sets.update({k: v[:3] for k, v in H.hand_cases().items()})
    return sets


@pytest.fixture(scope="module")
def runs(nat):
    """every set through the kernel ONCE: name -> dict(dt, gt, ids, images (the restatement's tables by image id),
    parsed result table, the OKS part of scratch, the host CSR table)"""
    from rtpe import scoring
    out = {}
    for name, (dt, gt, ids) in _sets().items():
        g = scoring.CocoKeypointGT(H.coco_dict(gt, ids))
        rec = _records(dt)
        result, scratch, tab = scoring._launch(rec, g)
        torch.cuda.synchronize()
        images = {i: SR.evaluate_image(*dt[i], gt.get(i, [])) for i in dt}
        mat = scratch[:max(tab["total"], 1) * D * 8].cpu().numpy().view(np.float64)
        out[name] = dict(dt=dt, gt=gt, ids=ids, g=g, rec=rec, images=images, raw=result.cpu().numpy(),
                         parsed=scoring.parse_result(result.cpu().numpy()), mat=mat, table=g.table())
    return out


def _kernel_matrix(run, image_id, n_dt):
    ids, offsets, _ = run["table"]
    k = int(np.searchsorted(ids, image_id))
    if k >= len(ids) or ids[k] != image_id:
        return np.zeros((n_dt, 0))
    o, G = int(offsets[k]), int(offsets[k + 1] - offsets[k])
    return run["mat"][o * D:o * D + n_dt * G].reshape(n_dt, G)


# ---- 1. the OKS matrix ------------------------------------------------------------------------------------------------
def test_oks_matrix_within_the_derived_bound(runs):
    worst, pairs, exact_ones, shapes = 0.0, 0, 0, set()
    for name, run in runs.items():
        for i, im in run["images"].items():
            want = im["oks"]
            got = _kernel_matrix(run, i, want.shape[0])
            assert got.shape == want.shape, (name, i)
            shapes.add(want.shape)
            if want.size:
                worst = max(worst, float(np.abs(got - want).max()))
                assert np.array_equal(got == 1.0, want == 1.0), (name, i)         # exact inputs give exact 1.0
                exact_ones += int((want == 1.0).sum())
                pairs += want.size
    print("OKS: %d pairs, max |kernel - restatement| = %.3e (bound %.3e), %d exact 1.0" % (pairs, worst, OKS_BOUND,
                                                                                          exact_ones))
    assert {(20, 40), (3, 2), (1, 1), (0, 1), (1, 0), (20, 2)} <= shapes           # 40 annotations: the scratch branch
    assert exact_ones >= 8 and pairs >= 2 * 20 * 40 + 20 * 2 + 3 * 2
    assert worst <= OKS_BOUND


def test_device_exp_against_numpy_exp(nat):
    """one visible joint and count 1: OKS = exp(-e) / 1 with e the restatement's own float64 value, so the kernel's
    OKS against ``np.exp(-e)`` is the distance of the two exps.  Seeded e in [0, 40]; the distance in units of the
    last place is printed and may not exceed the sum of the two documented errors."""
    from rtpe import scoring
    rng = np.random.default_rng(5)
    v = np.zeros(H.J)
    v[3] = 2
    base = H.pose()
    gt, dt = {}, {}
    for i in range(1, 13):
        gt[i] = [H.ann_of(base, 5000.0, v=v)]
        people = []
        for _ in range(20):
            p = base.copy()
            u = rng.uniform(0, 40)
            p[3, 0] += np.float32(np.sqrt(u * 2 * 5000.0 * (2 * SR.SIGMAS[3]) ** 2))
            people.append(p)
        dt[i] = (H.people_of(*people), np.linspace(1, .05, 20).astype(np.float32))
    g = scoring.CocoKeypointGT(H.coco_dict(gt))
    _, scratch, tab = scoring._launch(_records(dt), g)
    got = scratch[:tab["total"] * D * 8].cpu().numpy().view(np.float64).reshape(12, D)
    want = np.array([[SR.oks(p, gt[i][0]) for p in dt[i][0]] for i in range(1, 13)])
    e = -np.log(want)
    assert e.min() >= 0 and e.max() < 41 and (np.diff(np.sort(e.ravel())) > 0).all()
    ulps = np.abs(got - want) / np.spacing(want)
    print("exp: %d arguments in [%.3f, %.3f], max distance %.2f ulp, %d of them differ" % (
        e.size, -e.max(), -e.min(), ulps.max(), int((ulps > 0).sum())))
    assert ulps.max() <= EXP_ULPS_DEVICE + EXP_ULPS_NUMPY


# ---- 2. the match tables ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_sets()))
def test_match_tables_equal_the_restatement(runs, name):
    run = runs[name]
    ids, n_dt, scores, matched, ignored = run["parsed"]
    assert ids.tolist() == list(run["dt"])                                  # one row per record, in record order
    for k, i in enumerate(ids):
        im = run["images"][int(i)]
        n = len(im["order"])
        assert n_dt[k] == n == min(len(run["dt"][int(i)][1]), D)
        assert np.array_equal(scores[k, :n], im["scores"]) and not scores[k, n:].any()
        assert np.array_equal(matched[k, :, :, :n], im["matched"]), (name, i)
        assert np.array_equal(ignored[k, :, :, :n], im["ignored"]), (name, i)
        assert not matched[k, :, :, n:].any() and not ignored[k, :, :, n:].any()
    if name == "seeded":
        assert matched.any() and ignored.any() and (matched & ~ignored).any() and (~matched[:, :, 0] & ignored[:, :, 0]).sum() == 0


# ---- 3. the ten statistics --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_sets()))
def test_score_records_gives_the_ten_statistics(runs, name):
    from rtpe import scoring
    run = runs[name]
    got = scoring.score_records(run["rec"], run["g"])
    assert list(got) == list(SR.NAMES) and all(isinstance(v, float) for v in got.values())
    print(name, dict(got))
    if name == "seeded":
        assert got == SR.score(run["dt"], run["gt"], run["ids"])
    else:
        want = H.hand_cases()[name][3]
        for k in SR.NAMES:
            assert abs(got[k] - want[k]) <= 1e-12, (name, k, got[k], want[k])


def test_score_records_refuses_two_records_of_one_image(runs):
    from rtpe import scoring
    run = runs["exact"]
    twice = torch.cat([run["rec"], run["rec"][:1]])
    with pytest.raises(ValueError, match="more than one record"):
        scoring.score_records(twice, run["g"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.score_records(run["rec"].cpu(), run["g"])


# ---- 4. the result rows -----------------------------------------------------------------------------------------------
def test_every_byte_of_the_rows_is_written_and_nothing_else(runs):
    from rtpe import scoring
    run = runs["seeded"]
    want = run["raw"]
    n, row = want.shape
    assert row == 1288
    guard, sb = 256, run["g"].to(DEV)["total"] * (D * 8 + 4 + 30)
    sb = (sb + 7) // 8 * 8
    for fill in (0xA5, 0x00, 0xFF):
        res = torch.full((guard + n * row + guard,), fill, dtype=torch.uint8, device=DEV)
        scr = torch.full((guard + sb + guard,), fill, dtype=torch.uint8, device=DEV)
        for _ in range(2):                                                  # the second call finds a dirty buffer
            scoring._launch(run["rec"], run["g"], result=res[guard:guard + n * row], scratch=scr[guard:guard + sb])
            got = res.cpu().numpy()
            assert (got[:guard] == fill).all() and (got[-guard:] == fill).all()
            assert np.array_equal(got[guard:-guard].reshape(n, row), want)
            s = scr.cpu().numpy()
            assert (s[:guard] == fill).all() and (s[-guard:] == fill).all()
    # the bytes of a row, spelt out: header, scores, the two tables, nothing behind them at (10, 3, 20)
    assert 8 + 4 * D + 2 * 10 * 3 * D == row


# ---- 5. end to end ----------------------------------------------------------------------------------------------------
class _StandIn(torch.nn.Module):
    """a dual-head student that returns prepared maps: (att, det)"""

    def __init__(self, det):
        super().__init__()
        self.det = det

    def forward(self, x, alt=None):
        det = self.det[:x.shape[0]].clone()
        return det[:, :1].sigmoid(), det


class _OneByOne(torch.nn.Module):
    """the same maps one image per call, in order, for ``eval_student``'s loop"""

    def __init__(self, det):
        super().__init__()
        self.det, self.calls = det, 0

    def forward(self, img):
        d = self.det[self.calls:self.calls + 1].clone()
        self.calls += 1
        return d[:, :1].sigmoid(), d


def _annotations_of(dt, shift=0.0):
    gt = {}
    for i, (people, _) in dt.items():
        gt[i] = []
        for p in people:
            q = p.copy()
            q[:, 0] += np.float32(shift)
            q[:, 1] -= np.float32(shift / 2)
            gt[i].append(H.ann_of(q, max(SR.detection_area(p), 1500.0), v=np.where(p[:, 2] > 0, 2, 0)))
    return gt


def test_pipeline_records_to_the_reference_dict(nat):
    import socket
    import torch.distributed as dist
    from rtpe import engine, scoring
    det = _det((24, 32), (51, 52)).to(DEV)
    hw, ids = (96, 128), [9, 5]
    x = torch.zeros((2, 3) + hw, device=DEV)
    pipe = engine.StudentPipeline(_StandIn(det), _parser("device"), DEV, match_on="device")
    rec = pipe(x, image_ids=ids)
    dt = engine.unpack_records(rec)
    assert sorted(dt) == [5, 9] and sum(len(s) for _, s in dt.values()) >= 4

    exact = _annotations_of(dt)
    g = scoring.CocoKeypointGT(H.coco_dict(exact, ids))
    got = scoring.score_records(rec, g)
    assert got == SR.score(dt, exact, ids)
    for k in ("AP", "Ap .5", "AP .75", "AR", "AR .5", "AR .75"):
        assert got[k] == 1.0, got
    assert all(v in (1.0, -1.0) for v in got.values())

    for shift in (3.0, 6.0):
        moved = _annotations_of(dt, shift)
        gm = scoring.CocoKeypointGT(H.coco_dict(moved, ids))
        got_m = scoring.score_records(rec, gm)
        assert got_m == SR.score(dt, moved, ids)
    assert got_m["AP"] < 1.0                                               # 6 pixels cost something

    # eval_student over a two-item loader whose dataset is the annotations: the reference's dict
    class _Loader(list):
        dataset = g
    loader = _Loader([(ids[0], x[:1].cpu()), (ids[1], x[:1].cpu())])
    assert list(engine.eval_student(_OneByOne(det), _parser("host"), list(loader), DEV)) == ["images", "people"]
    got_e = engine.eval_student(_OneByOne(det), _parser("host"), loader, DEV)      # (a plain list has no dataset)
    assert list(got_e) == list(scoring.STAT_NAMES) and got_e == got

    # a one-rank gather of the record tensor scores the same
    assert not dist.is_initialized()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device(DEV))
    try:
        gathered = pipe.gather(None, rec, force_collective=True)
        assert gathered.is_cuda and scoring.score_records(gathered, g) == got
    finally:
        dist.destroy_process_group()
