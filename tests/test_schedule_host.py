"""The happens-before checker (oracle/schedule.py) sees every seeded fault - no GPU.

Hand-built programs of 4 to 10 ops on up to four lanes, each with a known answer; their traces are written by
``engine_trace`` below, which restates the executor's rules (mark_lane_waits, Lanes::stream_for / after / join of
csrc/engine.hip) for programs that no GPU is there to run.  The unmutated trace of every case gives no finding; every site
of every seeded fault (``schedule.MUTATIONS``) gives a finding that names the pair the fault leaves unordered.  The
same faults are seeded into the committed trace of a real teacher forward (tests/golden/lane_trace_teacher_64.json),
where a site may be harmless - a wait that another wait implies - so there some site of each fault must be caught.

The rules that need no trace (program-order lifetimes per slot with the promised pairs, the region rule) run on the
real programs: the teacher in fp16 and fp32, AttentionStudent with both bodies, AttentionStudentSteps."""
import copy
import json
import os
import re

import pytest

from oracle import schedule as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lane_trace_teacher_64.json")


# --------------------------------------------------------------------------- #
# the executor's rules, restated for hand-built programs
# --------------------------------------------------------------------------- #
def engine_trace(ops, routes):
    n = len(ops)
    cross = lambda j, d: ops[j]["region"] == d["region"] and d["region"] > 0 and ops[j]["lane"] != d["lane"]
    writer, readers, needs, waits = {}, {}, set(), [[] for _ in ops]
    for i, d in enumerate(ops):         # mark_lane_waits: per tensor id
        reads = ([d["in_t"]] if d["kind"] != S.OP_FUSE and d["in_t"] >= 0 else []) + ([d["res_t"]] if d["res_t"] >= 0 else []) + \
            d["term_t"][:d["n_terms"]]
        for t in reads + ([d["out_t"]] if d["out_t"] >= 0 else []):
            j = writer.get(t)
            if j is not None and cross(j, d):
                needs.add(j)
                waits[i].append(j)
        if d["out_t"] >= 0:
            for j in readers.get(d["out_t"], []):
                if j != i and cross(j, d):
                    needs.add(j)
                    waits[i].append(j)
            readers[d["out_t"]] = []
        for t in reads:
            readers.setdefault(t, []).append(i)
        if d["out_t"] >= 0:
            writer[d["out_t"]] = i
    trace, region, used = [], 0, set()

    def join():
        for lane in sorted(used):
            trace.append([S.RECORD, lane, n + lane, 0, 0])
            trace.append([S.WAIT, 0, n + lane, 0, 0])
        used.clear()

    for i, d in enumerate(ops):         # Lanes
        s = 0
        if d["region"] != region:
            join()
            region = d["region"]
            if region > 0:
                trace.append([S.RECORD, 0, n + S.FORK_EVENT, 0, 0])
                trace.extend([S.WAIT, lane, n + S.FORK_EVENT, 0, 0] for lane in (1, 2, 3))
        if region > 0:
            if d["lane"] > 0:
                s = d["lane"]
                used.add(s)
            j = i
            while j == i or (j < n and routes[j] == (S.ROUTE_DONE_BY, i)):
                trace.extend([S.WAIT, s, w, 0, 0] for w in waits[j])
                j += 1
        trace.append([S.LAUNCH, i, s, routes[i][0], routes[i][1]])
        if region > 0:
            if i in needs and routes[i][0] != S.ROUTE_PAIR_HEAD:
                trace.append([S.RECORD, s, i, 0, 0])
            if routes[i][0] == S.ROUTE_PAIR_TAIL and routes[i][1] in needs:
                trace.append([S.RECORD, s, routes[i][1], 0, 0])
    join()
    return trace


def conv(i, o, cin=48, cout=48, lane=0, region=0, **kw):
    return S.op_desc(S.OP_CONV, in_t=i, out_t=o, cin=cin, cout=cout, ksize=3, lane=lane, region=region, **kw)


def stem(o):
    return S.op_desc(S.OP_STEM, out_t=o, cin=3, cout=64, ksize=3, stride=2)


def fuse(terms, o, lane=0, region=0, cout=48):
    return S.op_desc(S.OP_FUSE, in_t=terms[0], out_t=o, cout=cout, n_terms=len(terms), term_t=(list(terms) + [0] * 4)[:4], lane=lane,
                     region=region)


def tensors_of(n, channels=64, slots=None):
    return [{"channels": channels, "ds_log2": 1, "slot": t if slots is None else slots.get(t, t), "esize": 2} for t in range(n)]


def case(ops, tensors, routes=None):
    routes = S.promised_routes(ops, pairs=False) if routes is None else routes
    return {"ops": ops, "tensors": tensors, "trace": engine_trace(ops, [tuple(r) for r in routes])}


def case_raw():
    """a read-after-write across lanes: op 3 (lane 0) reads what op 1 (lane 1) wrote"""
    ops = [stem(0), conv(0, 1, 64, 48, lane=1, region=1), conv(0, 2, 64, 48, region=1), conv(1, 3, region=1),
           fuse([2, 3], 4, region=1), conv(4, 5)]
    return case(ops, tensors_of(6))


def case_war():
    """a write-after-read into a shared `into=` tensor: op 4 (lane 0) overwrites tensor 1, which op 2 (lane 1) reads"""
    ops = [stem(0), conv(0, 1, 64, 48), conv(1, 2, lane=1, region=1), conv(0, 3, 64, 48, region=1), fuse([3, 0], 1, region=1),
           conv(1, 5), conv(2, 6)]
    return case(ops, tensors_of(7))


def case_concat():
    """two writers of disjoint channel slices of one concat tensor (2) on two lanes"""
    ops = [stem(0), conv(0, 1, 64, 48), conv(1, 2, lane=0, region=1, reserved=[0, 0, 48]),
           conv(0, 2, 64, 48, lane=1, region=1, out_coff=48, reserved=[0, 0, 48]), conv(2, 3, 96, 48)]
    ts = tensors_of(4)
    ts[2]["channels"] = 96
    return case(ops, ts)


def case_s2_group():
    """a stride-2 group (ops 4, 5: one launch at op 4) whose second member writes tensor 2, which op 3 of lane 1 reads"""
    s2 = dict(ksize=3, stride=2)
    ops = [stem(0), conv(0, 1, 64, 48), conv(0, 2, 64, 48), conv(2, 3, lane=1, region=1),
           S.op_desc(S.OP_CONV, in_t=1, out_t=4, cin=48, cout=48, region=1, **s2),
           S.op_desc(S.OP_CONV, in_t=1, out_t=2, cin=48, cout=48, region=1, **s2), conv(4, 6, region=1), conv(2, 7), conv(6, 8),
           conv(3, 9)]
    routes = S.promised_routes(ops, pairs=False)
    routes[4], routes[5] = (S.ROUTE_S2_GROUP, 2), (S.ROUTE_DONE_BY, 4)
    return case(ops, tensors_of(10), routes)


def pair_ops(region=0, lane=0):
    """0 stem, 1 the skip projection p (tensor 0 -> 1), 2 and 3 two convs, 4 the head (3 -> 4, residual 1), 5 the tail (4 -> 5)"""
    plain = 1 | 2
    return [stem(0), S.op_desc(S.OP_CONV, in_t=0, out_t=1, cin=64, cout=256, flags=2 | S.F_PAIR_PROJ), conv(0, 2, 64, 64),
            conv(2, 3, 64, 64),
            S.op_desc(S.OP_CONV, in_t=3, out_t=4, res_t=1, cin=64, cout=256, flags=plain | S.F_PAIR_HEAD, lane=lane, region=region),
            S.op_desc(S.OP_CONV, in_t=4, out_t=5, cin=256, cout=64, flags=plain | S.F_PAIR_TAIL, lane=lane, region=region)]


def case_pair_proj(reuse_after):
    """a pair with a folded projection; tensor 0, the projection's input, hands its slot on right after the tail (op 6's
    output, clean) or right after the head (the tail's output, a finding)"""
    ops = pair_ops() + [conv(5, 6, 64, 64), conv(6, 7, 64, 64)]
    ts = tensors_of(8, channels=256, slots={6: 0} if reuse_after == "tail" else {5: 0})
    return case(ops, ts, S.promised_routes(ops, pairs=True))


def case_pair_lane():
    """a 1x1 pair on lane 1 whose head's output (tensor 4) op 6 of lane 0 reads: the head's event belongs behind the tail"""
    ops = pair_ops(region=1, lane=1)
    ops[1]["flags"] = 2                 # (a plain residual: the projection runs as a conv of its own)
    ops += [conv(4, 6, 256, 64, region=1), conv(5, 7, 64, 64), conv(6, 8, 64, 64)]
    return case(ops, tensors_of(9, channels=256), S.promised_routes(ops, pairs=True))


def case_region_then_reuse():
    """a region followed by an op (5) whose output takes the slot of tensor 1, which lane 1 read inside the region"""
    ops = [stem(0), conv(0, 1, 64, 48), conv(1, 2, lane=1, region=1), conv(0, 3, 64, 48, region=1), fuse([3, 0], 4, region=1),
           conv(4, 5), conv(5, 6), conv(2, 7)]
    return case(ops, tensors_of(8, slots={5: 1}))


CASES = {"raw": case_raw, "war": case_war, "concat": case_concat, "s2_group": case_s2_group,
         "pair_proj": lambda: case_pair_proj("tail"), "pair_lane": case_pair_lane, "region_reuse": case_region_then_reuse}
# the seeded faults that have a site in each case (checked both ways: a case yields exactly these)
SITES = {
    "raw": {"drop_wait", "drop_record", "record_before_launch", "drop_fork_wait", "drop_join", "share_slot", "swap_conflicting_ops"},
    "war": {"drop_wait", "drop_record", "record_before_launch", "drop_fork_wait", "drop_join", "share_slot", "swap_conflicting_ops"},
    "concat": {"drop_wait", "drop_record", "record_before_launch", "drop_fork_wait", "drop_join", "share_slot", "swap_conflicting_ops"},
    "s2_group": {"drop_wait", "drop_record", "record_before_launch", "member_wait_at_member", "drop_fork_wait", "drop_join",
                 "share_slot", "swap_conflicting_ops"},
    "pair_proj": {"share_slot", "proj_input_ends_at_head"},
    "pair_lane": {"drop_wait", "drop_record", "record_before_launch", "pair_record_at_head", "drop_fork_wait", "drop_join",
                  "share_slot", "swap_conflicting_ops"},
    "region_reuse": {"drop_fork_wait", "drop_join", "share_slot"},
}
# sites that leave the schedule ordered, by construction: the two writers of the concat case touch disjoint channels, so
# the write-after-write wait that the executor derives per tensor id is an extra edge
HARMLESS = {("concat", "drop_wait"), ("concat", "record_before_launch"), ("concat", "swap_conflicting_ops"),
            # ... lane 1 of the concat case waits for an op that the caller's stream launched behind the fork,
            ("concat", "drop_fork_wait"),
            # ... and where the lane's last launch has an event that the caller's stream waits for, the join adds nothing
            ("raw", "drop_join"), ("war", "drop_join"), ("s2_group", "drop_join"), ("pair_lane", "drop_join")}


def test_the_route_numbers_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "rtpe_hip_trace.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define RTPE_(\w+) (\d+)", hdr)}
    for name in ("TRACE_INTS", "ROUTE_TILE", "ROUTE_HEAD", "ROUTE_S2", "ROUTE_S2_GROUP", "ROUTE_DECONV_MERGED", "ROUTE_PAIR_HEAD",
                 "ROUTE_PAIR_TAIL", "ROUTE_PAIR_PROJ", "ROUTE_BLOCK", "ROUTE_STEM_FUSED", "ROUTE_STEM_CONV1", "ROUTE_STEM_PLAIN",
                 "ROUTE_DONE_BY"):
        assert defs[name] == getattr(S, name), name
    for name in ("LAUNCH", "RECORD", "WAIT", "MASK", "FORK_EVENT"):
        assert defs["TRACE_" + name] == getattr(S, name), name


def test_trace_symbols_are_declared_in_their_header_and_resolve():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native as built
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, hdr = strip("rtpe_hip.h"), strip("rtpe_hip_trace.h")
    assert len(re.findall(r'#include "rtpe_hip_trace.h"', main)) == 1 and "#define RTPE_FWD_TRACE 2u" in main
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"rtpe_hrnet_forward_aux_flags", "rtpe_hrnet_read_trace"} == set(built.EXPORTS_TRACE)
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR, built.EXPORTS_RECORDS,
             built.EXPORTS_TAGMEAN, built.EXPORTS_NOPROJ, built.EXPORTS_ANYSIZE, built.EXPORTS_MIXED, built.EXPORTS_MIXDEC)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2, 6, 5, 4, 4, 4]      # no change to the existing tables
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "rtpe_hip_trace.h":
            assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", strip(name))), name
    lib = built.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == built._SIGS_TRACE[name][1], name
    assert built._SIGS_TRACE["rtpe_hrnet_forward_aux_flags"][1][:-1] == built._SIGS["rtpe_hrnet_forward_aux"][1]
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4 and built.FWD_TRACE == 2
    # an unknown flag bit is refused before anything else is looked at; the known ones reach the argument checks
    args = (None, None, built.RTPE_DTYPE_F16, 1, 64, 64, None, None, built.RTPE_DTYPE_F32, None, 0, None)
    assert lib.rtpe_hrnet_forward_flags(*args, 4) == -1 and b"unknown flag bits 0x4" in lib.rtpe_last_error_string()
    assert lib.rtpe_hrnet_forward_flags(*args, 3) == -1 and b"null argument" in lib.rtpe_last_error_string()
    import ctypes
    n = ctypes.c_int32(-1)
    assert lib.rtpe_hrnet_read_trace(None, None, 0, ctypes.byref(n)) == -1 and b"read_trace" in lib.rtpe_last_error_string()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_cases_are_clean(name):
    c = CASES[name]()
    assert 4 <= len(c["ops"]) <= 10
    findings = S.check(c["ops"], c["tensors"], c["trace"])
    assert findings == [], [f["text"] for f in findings]
    assert S.check_program(c["ops"], c["tensors"]) == []
    if name != "pair_proj":
        st = S.structure(c["ops"], c["tensors"], c["trace"])
        assert st["lane_launches"] >= 1 and st["waits"] > 3 and st["records"] >= 2, st


def test_hand_built_cases_hold_the_structures_they_are_named_for():
    st = {k: S.structure(c["ops"], c["tensors"], c["trace"]) for k, c in ((k, f()) for k, f in CASES.items())}
    assert st["raw"]["raw_waits"] == 1 and st["war"]["war_waits"] == 1 and st["concat"]["waw_waits"] == 1
    assert st["s2_group"]["s2_groups"] == 1 and st["s2_group"]["war_waits"] == 1
    assert st["pair_proj"]["pair_tails"] == 1 and st["pair_lane"]["pair_tails"] == 1 and st["pair_lane"]["raw_waits"] == 1
    c = CASES["pair_proj"]()
    assert S.routes_of(c["trace"], 8)[1] == (S.ROUTE_PAIR_PROJ, 5)


def test_disjoint_slices_of_a_concat_tensor_do_not_conflict():
    """without the write-after-write wait too: the checker works per channel range, the executor per tensor id"""
    c = CASES["concat"]()
    bare = [r for r in c["trace"] if not (r[0] == S.WAIT and r[2] < len(c["ops"]))]
    assert len(bare) == len(c["trace"]) - 1
    assert S.check(c["ops"], c["tensors"], bare) == []
    c["ops"][3]["out_coff"] = 32        # overlapping slices do
    f = S.check(c["ops"], c["tensors"], bare)
    assert [(x["rule"], x["op_a"], x["op_b"], x["tensor_a"], x["stream_a"], x["stream_b"]) for x in f] == [("race", 2, 3, 2, 0, 1)]
    assert "launch at op 2 on stream 0 -> launch at op 3 on stream 1" == f[0]["missing"]


def test_a_projection_input_reused_right_after_the_head_is_a_finding():
    c = case_pair_proj("head")
    f = S.check(c["ops"], c["tensors"], c["trace"])
    assert [(x["rule"], x["op_a"], x["op_b"], x["tensor_a"], x["tensor_b"], x["slot"]) for x in f] == [("same_launch", 5, 1, 5, 0, 0)]    # (the tail's write, the projection's read at the tail)
    assert any(x["rule"] == "same_launch" and {x["op_a"], x["op_b"]} == {1, 5} for x in S.check_program(c["ops"], c["tensors"]))
    # ... and without the fold the same slots are fine op by op: the projection has read tensor 0 long before the tail
    assert S.check(c["ops"], c["tensors"], S.one_stream_trace(S.promised_routes(c["ops"], pairs=False))) == []


def test_a_slot_reused_inside_a_region_is_a_finding_of_the_region_rule():
    c = case_region_then_reuse()
    ts = copy.deepcopy(c["tensors"])
    ts[3]["slot"] = ts[1]["slot"]       # tensor 3 (written by lane 0 in the region) into the slot of tensor 1 (read by lane 1)
    f = S.check_program(c["ops"], ts)
    assert any(x["rule"] == "regions" and (x["tensor_a"], x["tensor_b"]) == (1, 3) for x in f), f
    f = S.check(c["ops"], ts, c["trace"])
    assert any(x["rule"] == "race" and {x["op_a"], x["op_b"]} == {2, 3} and {x["stream_a"], x["stream_b"]} == {0, 1} for x in f), f


def test_a_wait_without_a_record_in_this_forward_orders_nothing():
    c = case_raw()
    k = next(k for k, r in enumerate(c["trace"]) if r[0] == S.RECORD and r[2] == 1)
    late = c["trace"][:k] + c["trace"][k + 1:] + [c["trace"][k]]        # the record comes, but behind the wait
    f = S.check(c["ops"], c["tensors"], late)
    assert any(x["rule"] == "unbound_wait" and x["event"] == 1 and x["op_b"] == 3 for x in f)
    assert any(x["rule"] == "race" and (x["op_a"], x["op_b"]) == (1, 3) for x in f)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_every_seeded_fault_is_caught_on_the_hand_built_cases(name, mutation):
    c = CASES[name]()
    sites = list(S.mutate(c["ops"], c["tensors"], c["trace"], mutation))
    assert bool(sites) == (mutation in SITES[name]), (name, mutation, [s[0] for s in sites])
    for label, ops, tensors, trace, expect in sites:
        findings = S.check(ops, tensors, trace)
        if (name, mutation) in HARMLESS:
            assert findings == [], (label, [f["text"] for f in findings])
            continue
        assert any(expect(f) for f in findings), (name, mutation, label, [f["text"] for f in findings])
        for f in findings:
            assert f["missing"] and f["text"] and f["stream_a"] is not None


def test_every_seeded_fault_has_a_hand_built_site():
    assert set().union(*SITES.values()) == set(S.MUTATIONS)


# --------------------------------------------------------------------------- #
# the committed trace of a real forward
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def real():
    with open(GOLDEN) as f:
        return json.load(f)


# what the real programs never contain (test_schedule_gpu.py names them too): no pair head inside a region whose output
# another lane reads, no group member with a wait that the group's first op does not have as well
NO_REAL_SITE = {"pair_record_at_head", "member_wait_at_member"}


def test_the_real_trace_is_clean_and_not_vacuous(real):
    ops, tensors, trace = real["ops"], real["tensors"], real["trace"]
    findings = S.check(ops, tensors, trace)
    assert findings == [], [f["text"] for f in findings[:8]]
    st = S.structure(ops, tensors, trace)
    print("structure of the committed trace:", st)
    assert st["raw_waits"] >= 1 and st["s2_groups"] >= 1 and st["proj_from_lane1"] >= 1 and st["regions_4_streams"] >= 1, st
    assert st["lane_launches"] >= 1


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_every_seeded_fault_is_caught_on_the_real_trace(real, mutation):
    ops, tensors, trace = real["ops"], real["tensors"], real["trace"]
    sites = list(S.mutate(ops, tensors, trace, mutation, limit=10 if mutation == "share_slot" else None))   # (pairs of tensors: many)
    assert bool(sites) == (mutation not in NO_REAL_SITE), (mutation, len(sites))
    caught = 0
    for label, o, ts, tr, expect in sites:
        findings = S.check(o, ts, tr)
        if findings:                    # a site that changes anything names the right pair
            assert any(expect(f) for f in findings), (mutation, label, [f["text"] for f in findings[:6]])
            caught += 1
    print("%s: %d of %d sites caught (the others are implied by another edge)" % (mutation, caught, len(sites)))
    if mutation == "drop_join" and caught == 0:
        # In the committed trace no join is the only edge from its lane: the last launch of every lane in every region has
        # an event that the caller's stream waits for in front of the join (the fuse sums run on lane 0 and read every
        # branch).  Shown here from the records alone; test_hand_built "region_reuse" has the join that matters.
        n = len(ops)
        for k, r in enumerate(trace):
            if r[0] == S.RECORD and n < r[2] < n + S.FORK_EVENT:
                lane = r[1]
                fork = max(j for j in range(k) if trace[j][0] == S.RECORD and trace[j][2] == n + S.FORK_EVENT)
                mine = [j for j in range(fork, k) if trace[j][0] == S.LAUNCH and trace[j][2] == lane and trace[j][3] not in S.NO_LAUNCH]
                if mine:
                    rec = [j for j in range(mine[-1], k) if trace[j][0] == S.RECORD and trace[j][1] == lane and trace[j][2] < n]
                    assert rec and any(trace[j][0] == S.WAIT and trace[j][1] == 0 and trace[j][2] == trace[rec[0]][2]
                                       for j in range(rec[0], k)), (lane, k)
        return
    assert caught >= 1 or not sites, mutation


# --------------------------------------------------------------------------- #
# the real programs, without a trace
# --------------------------------------------------------------------------- #
def _programs():
    import torch
    from rtpe import students
    from rtpe.helpers import build_hrnet_w48_teacher
    teacher = build_hrnet_w48_teacher()[1]
    yield "teacher fp16", teacher.compile_program()
    yield "teacher fp32", build_hrnet_w48_teacher()[1].float().compile_program()
    for name, model in students_models(students, torch):
        yield name, model.compile_program()


def students_models(students, torch):
    yield "AttentionStudent fp32 body", students.AttentionStudent(None, "cpu", 100, 17, 1, True, None, False).eval()
    yield "AttentionStudent half body", students.AttentionStudent(None, "cpu", 100, 17, 1, True, None, False, body_half=True).eval()
    yield "AttentionStudentSteps", students.AttentionStudentSteps(None, "cpu", 48, 17, 1, True, None, False).eval()


def test_real_programs_keep_their_slot_lifetimes_in_program_order():
    seen = []
    for name, prog in _programs():
        ops, tensors = S.descs(prog)
        findings = S.check_program(ops, tensors)
        assert findings == [], (name, [f["text"] for f in findings[:8]])
        seen.append((name, len(ops), len(set(t["slot"] for t in tensors)), sum(1 for d in ops if d["flags"] & S.F_PAIR_HEAD),
                     max(d["region"] for d in ops)))
    print(seen)
    by = dict((s[0], s) for s in seen)
    assert by["teacher fp16"][3] >= 1 and by["teacher fp16"][4] >= 2        # pairs and regions: the rules have something to do
    assert all(s[2] < s[1] for s in seen)                                    # slots are shared in every program
