"""Happens-before checker for one executor forward (plain Python: no torch, no GPU).

Input: the op and tensor descs of a ``Program`` (``descs``) and the trace of one forward (include/rtpe_hip_trace.h,
``Engine.read_trace``): LAUNCH / RECORD / WAIT records in the order in which the host enqueued them.  The checker
derives what every launch reads and writes from the descs and the route kinds alone - the table in ``launch_accesses``
is written from the kernels' argument setup in csrc/engine.hip ("What a launch touches") - builds the
happens-before relation of the trace and reports every pair of conflicting accesses that it leaves unordered, and every
workspace slot that is handed to another tensor while a reader of the first is still to come.

Happens-before
  - the records of one stream are ordered as enqueued;
  - a WAIT is ordered behind the latest RECORD of its event that was enqueued EARLIER IN THIS TRACE.  A wait that
    finds none contributes no edge (on the GPU it binds to the previous forward's record and orders nothing) and is
    reported (rule "unbound_wait");
  - the start of the caller's stream (stream 0) precedes everything, and everything must precede its end: a lane
    whose launch does not is reported (rule "unjoined").

Rules
  race          two accesses of different launches, at least one a write, to overlapping channel ranges of one
                tensor or to different tensors of one slot (a slot is one cell), not ordered
  same_launch   one launch writes a tensor and touches another tensor of the same slot
  overwritten   a read of T with a write to another tensor of T's slot between T's last write and the read
  regions       (``check_program`` only) two tensors of one slot touched inside one region by ops of different lanes
Extra edges are never an error.

A finding is a dict: rule, op_a / op_b (the ops whose operands collide, a before b in the trace), at_a / at_b (the ops
whose launches touch them), tensor_a / tensor_b, slot, stream_a / stream_b, missing (the edge that is not there), text.
"""
import copy

OP_STEM, OP_CONV, OP_DECONV, OP_FUSE, OP_CAST, OP_AVGPOOL, OP_SE, OP_CAM_COMBINE, OP_SIGMOID_ADD = range(9)
OP_AUX_PACK, OP_RESIZE, OP_GATE_MUL = 9, 10, 11
F_NO_NHWC, F_PAIR_HEAD, F_PAIR_TAIL, F_PAIR_PROJ = 16, 64, 128, 256
# include/rtpe_hip_trace.h (tests/test_schedule_host.py compares these with the header)
TRACE_INTS, LAUNCH, RECORD, WAIT, MASK, FORK_EVENT = 5, 1, 2, 3, 4, 4
ROUTE_NONE, ROUTE_TILE, ROUTE_HEAD, ROUTE_S2, ROUTE_S2_GROUP, ROUTE_DECONV_MERGED = 0, 1, 5, 6, 7, 8
ROUTE_PAIR_HEAD, ROUTE_PAIR_TAIL, ROUTE_PAIR_PROJ, ROUTE_BLOCK = 10, 11, 12, 13
ROUTE_STEM_FUSED, ROUTE_STEM_CONV1, ROUTE_STEM_PLAIN, ROUTE_DONE_BY = 14, 15, 16, 17
NO_LAUNCH = (ROUTE_DONE_BY, ROUTE_PAIR_HEAD, ROUTE_PAIR_PROJ)       # computed by the launch at op `by`

OP_FIELDS = ("kind", "flags", "in_t", "in_coff", "out_t", "out_coff", "res_t", "res_coff", "cin", "cout", "ksize",
             "stride", "n_terms", "term_t", "reserved", "lane", "region")


def descs(program):
    """(ops, tensors) of a compiled ``Program`` as lists of plain dicts (JSON-able)"""
    ops = [{k: ([int(v) for v in getattr(d, k)] if k in ("term_t", "reserved") else int(getattr(d, k))) for k in OP_FIELDS}
           for d in program.ops]
    tensors = [{"channels": int(t.channels), "ds_log2": int(t.ds_log2), "slot": int(t.slot), "esize": int(t.reserved)}
               for t in program.tensors]
    return ops, tensors


def op_desc(kind=OP_CONV, **kw):
    """an op desc for hand-built programs: the fields of OP_FIELDS, with the defaults of an op that touches nothing"""
    d = {"kind": kind, "flags": 0, "in_t": -1, "in_coff": 0, "out_t": -1, "out_coff": 0, "res_t": -1, "res_coff": 0, "cin": 0,
         "cout": 0, "ksize": 1, "stride": 1, "n_terms": 0, "term_t": [0, 0, 0, 0], "reserved": [0, 0, 0], "lane": 0, "region": 0}
    assert set(kw) <= set(d), set(kw) - set(d)
    d.update(kw)
    return d


# --------------------------------------------------------------------------- #
# what a launch touches
# --------------------------------------------------------------------------- #
def _span(tensors, t, lo, n):
    return (t, lo, min(lo + max(n, 1), tensors[t]["channels"]))


def op_reads(ops, tensors, i, inp=True, res=True):
    """[(tensor, lo, hi)] that op i reads when it runs as a launch of its own"""
    d, out = ops[i], []
    k = d["kind"]
    if k == OP_FUSE:                    # launch_fuse: the terms from channel 0, cout channels each; in_t is not read
        return [_span(tensors, d["term_t"][t], 0, d["cout"]) for t in range(d["n_terms"])]
    if inp and d["in_t"] >= 0 and k not in (OP_STEM, OP_AUX_PACK):      # (those two read the network's inputs)
        out.append(_span(tensors, d["in_t"], d["in_coff"], 1 if k in (OP_SIGMOID_ADD, OP_GATE_MUL) else
                         d["cout"] if k == OP_CAM_COMBINE else d["cin"]))
    if res and d["res_t"] >= 0 and k not in (OP_SE, OP_AVGPOOL):
        out.append(_span(tensors, d["res_t"], d["res_coff"], d["cout"]))
    if k == OP_CAM_COMBINE:             # the SE gate: one vector per image
        out.append(_span(tensors, d["term_t"][0], 0, d["cout"]))
    return out


def op_writes(ops, tensors, i):
    """[(tensor, lo, hi)] that op i writes to the workspace.  RTPE_F_NO_NHWC: nothing (the NCHW output only).  A conv
    stores its padded channels too, as far as the row has room: reserved[2] where it is set, else cout rounded up to 16
    (conv_op_args: cout_store; padding beyond a multiple of 16, which depends on the kernel's row tile, is not modelled:
    an op that writes beside a neighbour in a shared tensor sets reserved[2])."""
    d = ops[i]
    if d["out_t"] < 0 or (d["flags"] & F_NO_NHWC):
        return []
    n = d["cout"]
    if d["kind"] in (OP_CONV, OP_DECONV):
        n = d["reserved"][2] if d["reserved"][2] > 0 else (d["cout"] + 15) // 16 * 16
    if d["kind"] == OP_SE:
        n = d["cin"]
    return [_span(tensors, d["out_t"], d["out_coff"], n)]


def launch_accesses(ops, tensors, routes, i):
    """What the launch at op i touches, from the descs and the route kinds: [(op, tensor, lo, hi, "r" | "w")], `op` being
    the op whose operand it is.  routes[i] = (how, by).  Written from block_args / launch_block, conv_pair_launch,
    stem_fused_args, conv48s2_launch_group and conv_op_args of csrc/engine.hip:
      DONE_BY, PAIR_HEAD, PAIR_PROJ   nothing at the op's own place
      BLOCK at i        reads in(i), which is res(i + 1) too; writes out(i + 1); the inner tensor out(i) is neither
                        written nor read (it lives in LDS)
      STEM_FUSED at i   reads the image; writes out(i + 1); the stem's own output is not written
      S2_GROUP at i     reads and writes of ops i .. i + by - 1
      PAIR_TAIL at i    (head h = by) reads in(h) and res(h) - or, when an op p is routed PAIR_PROJ with by = i, in(p) instead
                        of res(h), whose tensor is then never written; writes out(h) and out(i); in(i) = out(h) is not read back
      anything else     the op's own reads and writes (a merged transposed conv: all channels of in, one launch)"""
    how, by = routes[i]
    acc = []

    def own(j, reads=True, writes=True, **kw):
        if reads:
            acc.extend((j,) + s + ("r",) for s in op_reads(ops, tensors, j, **kw))
        if writes:
            acc.extend((j,) + s + ("w",) for s in op_writes(ops, tensors, j))

    if how in NO_LAUNCH:
        return acc
    if how == ROUTE_BLOCK:
        own(i, writes=False)
        own(i + 1, inp=False)
    elif how == ROUTE_STEM_FUSED:
        own(i + 1, reads=False)
    elif how == ROUTE_S2_GROUP:
        for m in range(by):
            own(i + m)
    elif how == ROUTE_PAIR_TAIL:
        proj = [p for p, r in enumerate(routes) if r[0] == ROUTE_PAIR_PROJ and r[1] == i]
        own(by, res=not proj)
        for p in proj:
            own(p, writes=False)
        own(i, reads=False)
    else:
        own(i)
    return acc


def routes_of(trace, n_ops):
    routes = [(ROUTE_NONE, 0)] * n_ops
    for r in trace:
        if r[0] == LAUNCH:
            routes[r[1]] = (r[3], r[4])
    return routes


# --------------------------------------------------------------------------- #
# happens-before
# --------------------------------------------------------------------------- #
def _stream(r):
    return r[2] if r[0] == LAUNCH else r[1]


def order(trace):
    """anc[k] = bit set of the records that happen before record k; unbound = indices of waits without a record"""
    anc, last_on, last_rec, unbound = [0] * len(trace), {}, {}, []
    for k, r in enumerate(trace):
        m, p = 0, last_on.get(_stream(r))
        if p is not None:
            m |= anc[p] | (1 << p)
        if r[0] == WAIT:
            q = last_rec.get(r[2])
            if q is None:
                unbound.append(k)
            else:
                m |= anc[q] | (1 << q)
        if r[0] == RECORD:
            last_rec[r[2]] = k
        anc[k] = m
        last_on[_stream(r)] = k
    return anc, unbound


def _finding(rule, a, b, tensors, text, missing):
    """a, b: access tuples (node, at, stream, op, tensor, lo, hi, rw)"""
    return {"rule": rule, "op_a": a[3], "op_b": b[3], "at_a": a[1], "at_b": b[1], "tensor_a": a[4], "tensor_b": b[4],
            "slot": tensors[a[4]]["slot"], "stream_a": a[2], "stream_b": b[2], "missing": missing, "text": text}


def check(ops, tensors, trace):
    """the findings of one forward (an empty list: every conflicting pair is ordered)"""
    trace = [list(r) for r in trace]
    n_ops = len(ops)
    routes = routes_of(trace, n_ops)
    anc, unbound = order(trace)
    hb = lambda a, b: (anc[b] >> a) & 1
    findings = []
    launches = [k for k, r in enumerate(trace) if r[0] == LAUNCH]
    for k in unbound:
        nxt = [trace[j][1] for j in launches if j > k and trace[j][2] == trace[k][1]]
        ev = trace[k][2]
        findings.append({"rule": "unbound_wait", "op_a": ev if ev < n_ops else -1, "op_b": nxt[0] if nxt else -1, "at_a": -1,
                         "at_b": -1, "tensor_a": -1, "tensor_b": -1, "slot": -1, "stream_a": -1, "stream_b": trace[k][1],
                         "event": ev, "missing": "a record of event %d in front of the wait on stream %d" % (ev, trace[k][1]),
                         "text": "stream %d waits for event %d, which this forward has not recorded: the wait orders nothing"
                                 % (trace[k][1], ev)})
    acc = []                            # (node, at, stream, op, tensor, lo, hi, rw)
    for k in launches:
        _, i, s, how, by = trace[k]
        acc.extend((k, i, s) + a for a in launch_accesses(ops, tensors, routes, i))
    # everything precedes the end of the caller's stream
    on0 = [k for k, r in enumerate(trace) if _stream(r) == 0]
    end = (anc[on0[-1]] | (1 << on0[-1])) if on0 else 0
    loose = {}
    for k in launches:
        if trace[k][3] not in NO_LAUNCH and not (end >> k) & 1:
            loose.setdefault(trace[k][2], trace[k][1])
    for s, i in sorted(loose.items()):
        findings.append({"rule": "unjoined", "op_a": i, "op_b": -1, "at_a": i, "at_b": -1, "tensor_a": -1, "tensor_b": -1,
                         "slot": -1, "stream_a": s, "stream_b": 0, "missing": "a join of stream %d into stream 0 behind op %d" % (s, i),
                         "text": "op %d runs on stream %d, which the caller's stream never waits for afterwards" % (i, s)})
    by_slot = {}
    for a in acc:
        by_slot.setdefault(tensors[a[4]]["slot"], []).append(a)
    seen = set()

    def report(rule, a, b, text, missing):
        key = (rule, a[1], b[1], a[3], b[3], a[4], b[4])
        if key not in seen:
            seen.add(key)
            findings.append(_finding(rule, a, b, tensors, text, missing))

    for slot, group in sorted(by_slot.items()):
        writes = [a for a in group if a[7] == "w"]
        for x in writes:
            for y in group:
                if x is y or (y[7] == "w" and (y[0], y[3], y[4]) < (x[0], x[3], x[4])):          # (each pair of writes once)
                    continue
                same_t = x[4] == y[4]
                if same_t and not (x[5] < y[6] and y[5] < x[6]):
                    continue
                a, b = (x, y) if x[0] <= y[0] else (y, x)
                what = "tensor %d" % a[4] if same_t else "tensors %d and %d of slot %d" % (a[4], b[4], slot)
                if a[0] == b[0]:
                    if not same_t:
                        report("same_launch", a, b, "the launch at op %d %s tensor %d (op %d) and %s tensor %d (op %d) of slot %d"
                               % (a[1], "writes" if a[7] == "w" else "reads", a[4], a[3], "writes" if b[7] == "w" else "reads",
                                  b[4], b[3], slot), "tensors %d and %d in different slots" % (a[4], b[4]))
                    continue
                if not hb(a[0], b[0]):
                    report("race", a, b, "op %d (launched at op %d, stream %d) %s and op %d (launched at op %d, stream %d) %s %s, unordered"
                           % (a[3], a[1], a[2], "writes" if a[7] == "w" else "reads", b[3], b[1], b[2],
                              "writes" if b[7] == "w" else "reads", what),
                           "launch at op %d on stream %d -> launch at op %d on stream %d" % (a[1], a[2], b[1], b[2]))
        # a slot handed on too early: W(T) -> X(U) -> read(T) with no write of T between X and the read
        for r in group:
            if r[7] != "r":
                continue
            mine = [w for w in writes if w[4] == r[4] and w[5] < r[6] and r[5] < w[6]]
            for x in writes:
                if x[4] == r[4] or x[0] == r[0] or not hb(x[0], r[0]):
                    continue
                if any(hb(w[0], x[0]) for w in mine) and not any(hb(x[0], w[0]) and hb(w[0], r[0]) for w in mine):
                    report("overwritten", x, r, "op %d (launched at op %d) writes tensor %d into slot %d between the last write of "
                           "tensor %d and its read by op %d (launched at op %d)" % (x[3], x[1], x[4], slot, r[4], r[3], r[1]),
                           "tensor %d live until the launch at op %d (or tensor %d in another slot)" % (r[4], r[1], x[4]))
    return findings


# --------------------------------------------------------------------------- #
# the rules that need no trace
# --------------------------------------------------------------------------- #
def promised_routes(ops, pairs=True):
    """the routes a program's flags announce: every op a launch of its own; with `pairs`, the flagged 1x1 pairs as one
    launch at the tail and a flagged skip projection folded into it (include/rtpe_hip.h, RTPE_F_PAIR_HEAD / _PROJ)"""
    routes = [(ROUTE_STEM_PLAIN if d["kind"] == OP_STEM else ROUTE_TILE if d["kind"] in (OP_CONV, OP_DECONV) else ROUTE_NONE, 0)
              for d in ops]
    for i in range(len(ops) - 1 if pairs else 0):
        if ops[i]["flags"] & F_PAIR_HEAD and ops[i + 1]["flags"] & F_PAIR_TAIL:
            routes[i], routes[i + 1] = (ROUTE_PAIR_HEAD, i + 1), (ROUTE_PAIR_TAIL, i)
            for p in range(i):
                if ops[p]["flags"] & F_PAIR_PROJ and ops[p]["out_t"] == ops[i]["res_t"]:
                    routes[p] = (ROUTE_PAIR_PROJ, i + 1)
    return routes


def one_stream_trace(routes):
    return [[LAUNCH, i, 0, how, by] for i, (how, by) in enumerate(routes)]


def check_program(ops, tensors):
    """Program-order lifetimes per slot - every op on one stream, once as launches of their own and once with the
    promised pairs and folded projections - and the region rule: inside a region the lanes may run in any order, so two
    tensors of one slot must not both be touched there by ops of different lanes."""
    findings = []
    for pairs in (False, True):
        for f in check(ops, tensors, one_stream_trace(promised_routes(ops, pairs))):
            f["text"] = ("with the promised pairs: " if pairs else "op by op: ") + f["text"]
            if not any(all(g[k] == f[k] for k in ("rule", "op_a", "op_b", "tensor_a", "tensor_b")) for g in findings):
                findings.append(f)
    touched = {}                        # region -> tensor -> (lanes, first op)
    plain = promised_routes(ops, False)
    for i, d in enumerate(ops):
        if d["region"] > 0:
            for a in launch_accesses(ops, tensors, plain, i):
                lanes, _ = touched.setdefault(d["region"], {}).setdefault(a[1], (set(), i))
                lanes.add(d["lane"])
    for region, ts in sorted(touched.items()):
        for t in sorted(ts):
            for u in sorted(ts):
                if t < u and tensors[t]["slot"] == tensors[u]["slot"] and len(ts[t][0] | ts[u][0]) > 1:
                    findings.append({"rule": "regions", "op_a": ts[t][1], "op_b": ts[u][1], "at_a": ts[t][1], "at_b": ts[u][1],
                                     "tensor_a": t, "tensor_b": u, "slot": tensors[t]["slot"], "stream_a": min(ts[t][0]),
                                     "stream_b": min(ts[u][0]), "missing": "tensors %d and %d in different slots" % (t, u),
                                     "text": "tensors %d and %d share slot %d and are both touched inside region %d, by ops of lanes %s"
                                             % (t, u, tensors[t]["slot"], region, sorted(ts[t][0] | ts[u][0]))})
    return findings


# --------------------------------------------------------------------------- #
# structure counts (so that a clean result cannot be vacuous)
# --------------------------------------------------------------------------- #
def structure(ops, tensors, trace):
    """what a trace contains: lane launches, cross-lane waits by hazard, grouped stride-2 launches, pair tails with a
    projection folded from lane 1, regions with work on all four streams"""
    n_ops = len(ops)
    routes = routes_of(trace, n_ops)
    stream_of = {r[1]: r[2] for r in trace if r[0] == LAUNCH}
    out = {"launches": sum(1 for r in trace if r[0] == LAUNCH and r[3] not in NO_LAUNCH),
           "lane_launches": sum(1 for r in trace if r[0] == LAUNCH and r[2] > 0 and r[3] not in NO_LAUNCH),
           "waits": sum(1 for r in trace if r[0] == WAIT), "records": sum(1 for r in trace if r[0] == RECORD),
           "raw_waits": 0, "war_waits": 0, "waw_waits": 0,
           "s2_groups": sum(1 for how, by in routes if how == ROUTE_S2_GROUP),
           "pair_tails": sum(1 for how, by in routes if how == ROUTE_PAIR_TAIL), "proj_from_lane1": 0, "regions_4_streams": 0}
    for p, (how, by) in enumerate(routes):
        if how == ROUTE_PAIR_PROJ and routes[by][0] == ROUTE_PAIR_TAIL and ops[p]["lane"] == 1 and stream_of.get(p) == 1:
            out["proj_from_lane1"] += 1
    # a cross-lane wait, by what the waiting launch and the event's op do to a common tensor
    for k, r in enumerate(trace):
        if r[0] != WAIT or r[2] >= n_ops:
            continue
        nxt = [q for q in trace[k:] if q[0] == LAUNCH and q[2] == r[1] and q[3] not in NO_LAUNCH]
        if not nxt:
            continue
        w_src = set(t for t, _, _ in op_writes(ops, tensors, r[2]))
        r_src = set(t for t, _, _ in op_reads(ops, tensors, r[2]))
        mine = launch_accesses(ops, tensors, routes, nxt[0][1])
        if any(a[4] == "r" and a[1] in w_src for a in mine):
            out["raw_waits"] += 1
        elif any(a[4] == "w" and a[1] in w_src for a in mine):
            out["waw_waits"] += 1
        elif any(a[4] == "w" and a[1] in r_src for a in mine):
            out["war_waits"] += 1
    streams, region = set(), 0
    for r in trace:
        if r[0] != LAUNCH or r[3] in NO_LAUNCH:
            continue
        if ops[r[1]]["region"] != region:
            out["regions_4_streams"] += region > 0 and len(streams) == 4
            streams, region = set(), ops[r[1]]["region"]
        streams.add(r[2])
    out["regions_4_streams"] += region > 0 and len(streams) == 4
    return out


# --------------------------------------------------------------------------- #
# seeded faults
# --------------------------------------------------------------------------- #
MUTATIONS = ("drop_wait", "drop_record", "record_before_launch", "pair_record_at_head", "member_wait_at_member",
             "drop_fork_wait", "drop_join", "share_slot", "proj_input_ends_at_head", "swap_conflicting_ops")


def _computed_by(routes, i):
    """the ops whose bytes the launch at op i produces or whose operands it reads"""
    out = {i}
    how, by = routes[i]
    if how == ROUTE_S2_GROUP:
        out |= set(range(i, i + by))
    if how in (ROUTE_BLOCK, ROUTE_STEM_FUSED):
        out.add(i + 1)
    if how == ROUTE_PAIR_TAIL:
        out.add(by)
        out |= set(p for p, r in enumerate(routes) if r[0] == ROUTE_PAIR_PROJ and r[1] == i)
    return out


def _launch_node(trace, routes, op):
    """index of the LAUNCH record whose launch computes `op`"""
    how, by = routes[op]
    while how in NO_LAUNCH:
        op = by
        how, by = routes[op]
    return next(k for k, r in enumerate(trace) if r[0] == LAUNCH and r[1] == op)


def _next_launch(trace, k, stream):
    return next((j for j in range(k, len(trace)) if trace[j][0] == LAUNCH and trace[j][2] == stream and trace[j][3] not in NO_LAUNCH), None)


def mutate(ops, tensors, trace, name, limit=None):
    """The sites of seeded fault `name` in a case: yields (label, ops, tensors, trace, expect) with `expect` a predicate on one
    finding - true for a finding that names the pair the fault leaves unordered.  A case without the structure the fault
    needs yields nothing.  On a real trace a site may be harmless (a wait that another wait implies: extra edges are
    allowed), so a caller asks that SOME site of a mutation is caught there, and every site on the hand-built cases."""
    assert name in MUTATIONS
    n_ops = len(ops)
    routes = routes_of(trace, n_ops)
    count = [0]

    def site(label, tr=None, ts=None, expect=None):
        count[0] += 1
        return (label, ops, tensors if ts is None else ts, trace if tr is None else tr, expect)

    def full():
        return limit is not None and count[0] >= limit

    def pair(a_ops, b_ops):
        a_ops, b_ops = set(a_ops), set(b_ops)
        return lambda f: (f["op_a"] in a_ops and f["op_b"] in b_ops) or (f["op_a"] in b_ops and f["op_b"] in a_ops)

    op_waits = [k for k, r in enumerate(trace) if r[0] == WAIT and r[2] < n_ops]
    if name == "drop_wait":
        for k in op_waits:
            j = _next_launch(trace, k, trace[k][1])
            nxt = next(r for r in trace[k:] if r[0] == LAUNCH and r[2] == trace[k][1])
            if nxt[3] == ROUTE_DONE_BY:   # (the executor enqueues an absorbed op's waits at the launch that computes it AND at its own place)
                continue
            if j is not None and not full():
                yield site("wait %d (event of op %d, in front of op %d)" % (k, trace[k][2], trace[j][1]), trace[:k] + trace[k + 1:],
                           expect=pair([trace[k][2]], _computed_by(routes, trace[j][1])))
    elif name == "drop_record":
        for k, r in enumerate(trace):
            if r[0] == RECORD and r[2] < n_ops and any(trace[w][2] == r[2] for w in op_waits) and not full():
                yield site("record %d (event of op %d)" % (k, r[2]), trace[:k] + trace[k + 1:],
                           expect=lambda f, e=r[2]: f["rule"] == "unbound_wait" and f["event"] == e)
    elif name == "record_before_launch":
        for k, r in enumerate(trace):
            if r[0] == RECORD and r[2] < n_ops and not full():
                at = _launch_node(trace, routes, r[2])
                waiters = set()
                for w in op_waits:
                    j = _next_launch(trace, w, trace[w][1])
                    if trace[w][2] == r[2] and j is not None:
                        waiters |= _computed_by(routes, trace[j][1])
                if at < k and waiters:
                    yield site("record %d of op %d in front of launch %d" % (k, r[2], at),
                               trace[:at] + [trace[k]] + trace[at:k] + trace[k + 1:], expect=pair(_computed_by(routes, trace[at][1]), waiters))
    elif name == "pair_record_at_head":
        for k, r in enumerate(trace):
            if r[0] == RECORD and r[2] < n_ops and routes[r[2]][0] == ROUTE_PAIR_HEAD and not full():
                head = next(j for j, q in enumerate(trace) if q[0] == LAUNCH and q[1] == r[2])
                waiters = set()
                for w in op_waits:
                    j = _next_launch(trace, w, trace[w][1])
                    if trace[w][2] == r[2] and j is not None:
                        waiters |= _computed_by(routes, trace[j][1])
                yield site("record of pair head %d at the head" % r[2], trace[:head + 1] + [trace[k]] + trace[head + 1:k] + trace[k + 1:],
                           expect=pair([r[2]], waiters))
    elif name == "member_wait_at_member":
        for k in op_waits:
            j = _next_launch(trace, k, trace[k][1])
            if j is None or routes[trace[j][1]][0] not in (ROUTE_S2_GROUP, ROUTE_BLOCK, ROUTE_STEM_FUSED) or full():
                continue
            lead = trace[j][1]
            src_t = set(t for t, _, _ in op_reads(ops, tensors, trace[k][2]) + op_writes(ops, tensors, trace[k][2]))
            touch = lambda m: set(t for t, _, _ in op_reads(ops, tensors, m) + op_writes(ops, tensors, m))
            for m in sorted(_computed_by(routes, lead) - {lead}):
                if src_t & touch(m) and not src_t & touch(lead) and sum(1 for w in op_waits if trace[w][2] == trace[k][2] and w < j and trace[w][1] == trace[k][1]) == 1:
                    at_m = next(q for q, r in enumerate(trace) if r[0] == LAUNCH and r[1] == m)
                    yield site("wait %d for op %d moved from the group's launch at op %d to member %d" % (k, trace[k][2], lead, m),
                               trace[:k] + trace[k + 1:at_m] + [trace[k]] + trace[at_m:], expect=pair([trace[k][2]], [m]))
    elif name in ("drop_fork_wait", "drop_join"):
        forks = [k for k, r in enumerate(trace) if r[0] == RECORD and r[2] == n_ops + FORK_EVENT]
        for n, k in enumerate(forks):
            stop = forks[n + 1] if n + 1 < len(forks) else len(trace)
            before = set(trace[j][1] for j in range(k) if trace[j][0] == LAUNCH)
            for lane in (1, 2, 3):
                mine = set()
                for j in range(k, stop):
                    if trace[j][0] == LAUNCH and trace[j][2] == lane and trace[j][3] not in NO_LAUNCH:
                        mine |= _computed_by(routes, trace[j][1])
                if not mine or full():
                    continue
                if name == "drop_fork_wait":
                    w = next(j for j in range(k, stop) if trace[j][0] == WAIT and trace[j][1] == lane and trace[j][2] == n_ops + FORK_EVENT)
                    yield site("fork wait of lane %d at record %d" % (lane, w), trace[:w] + trace[w + 1:], expect=pair(before, mine))
                else:
                    jr = next(j for j in range(k, stop) if trace[j][0] == RECORD and trace[j][2] == n_ops + lane)
                    jw = next(j for j in range(jr, stop) if trace[j][0] == WAIT and trace[j][2] == n_ops + lane)
                    after = set(trace[j][1] for j in range(jw, len(trace)) if trace[j][0] == LAUNCH)
                    ok = pair(mine, after)
                    yield site("join of lane %d at records %d, %d" % (lane, jr, jw), [r for j, r in enumerate(trace) if j not in (jr, jw)],
                               expect=lambda f, ok=ok, lane=lane: ok(f) or (f["rule"] == "unjoined" and f["stream_a"] == lane))
    elif name == "share_slot":
        # T written at launch a and read at launch c, U written by a launch b between them: U moves into T's slot
        acc = []
        for k, r in enumerate(trace):
            if r[0] == LAUNCH:
                acc.extend((k,) + a for a in launch_accesses(ops, tensors, routes, r[1]))
        first_w, last_r = {}, {}
        for k, op, t, lo, hi, rw in acc:
            if rw == "w":
                first_w.setdefault(t, (k, op))
            else:
                last_r[t] = (k, op)
        for t in sorted(first_w):
            for u in sorted(first_w):
                if (t != u and t in last_r and tensors[t]["slot"] != tensors[u]["slot"] and first_w[t][0] < first_w[u][0] < last_r[t][0]
                        and not full()):
                    ts = copy.deepcopy(tensors)
                    ts[u]["slot"] = ts[t]["slot"]
                    users = lambda v: set(op for k, op, tt, lo, hi, rw in acc if tt == v)
                    yield site("tensor %d into the slot of tensor %d" % (u, t), ts=ts, expect=pair(users(u), users(t)))
    elif name == "proj_input_ends_at_head":
        for p, (how, by) in enumerate(routes):
            if how == ROUTE_PAIR_PROJ and not full():
                ts = copy.deepcopy(tensors)
                ts[ops[by]["out_t"]]["slot"] = ts[ops[p]["in_t"]]["slot"]
                yield site("the tail's output (op %d) into the slot of the projection's input (op %d)" % (by, p), ts=ts,
                           expect=pair([p, routes[by][1]], [by]))
    elif name == "swap_conflicting_ops":
        for k in op_waits:
            j = _next_launch(trace, k, trace[k][1])
            if j is None or full() or next(r for r in trace[k:] if r[0] == LAUNCH and r[2] == trace[k][1])[3] == ROUTE_DONE_BY:
                continue
            a = _launch_node(trace, routes, trace[k][2])
            if a < j and trace[a][2] != trace[j][2]:
                tr = list(trace)
                tr[a], tr[j] = trace[j], trace[a]
                yield site("launches of op %d (stream %d) and op %d (stream %d) swapped" % (trace[a][1], trace[a][2], trace[j][1], trace[j][2]),
                           tr, expect=pair(_computed_by(routes, trace[a][1]), _computed_by(routes, trace[j][1])))
