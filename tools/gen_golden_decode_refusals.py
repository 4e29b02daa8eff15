#!/usr/bin/env python3
"""Generate tests/golden/decode_refusals.json: what the thirteen network-output decode entries of csrc/decode.hip
(plain, `_shared`, `_sizes`, `_mixed`; top-k, adjust + refine, `_n`) and the two table fills answer to arguments they
refuse - or accept - BEFORE any launch, recorded from a built library, and the bytes the fills write on four shapes.
tests/test_decode_refusals_host.py replays the file against the library of the tree; no GPU is needed for either.

    python tools/gen_golden_decode_refusals.py                    # record from the tree's library
    python tools/gen_golden_decode_refusals.py --replay           # compare the tree's library with the file
    RTPE_LIBRARY=/path/to/librtpe_hip.so python tools/gen_golden_decode_refusals.py [--replay] [--messages FILE]

The grid.  Every entry has a base call with sound arguments; a fault changes one or two of them, and a call holds one
fault, or two whose own first messages differ.  Pointers are fake addresses (a tag times 0x10000): every call of the
grid returns before anything is dereferenced or launched, which was checked by reading the code, not by trying:

* adjust + refine entries: the base call has P = 0, which every kind accepts after its checks, before with_maps.  P = 1
  occurs only together with ans_in / ans_out null or equal, which decode_adjust_refine refuses for every kind.
* top-k entries: a sound call would launch, so every call holds a fault that the kind's check() or topk_check refuses.
  A fault that the kind does not look at (J = 33, a zero map size or a short image stride on the plain kind; J = 33
  and the strides on the `_sizes` kind) is recorded together with val_k = null, which topk_check refuses after
  check(): the first message then tells whether the kind looked.
* the fills get real arrays and a real table; they dereference nothing before their checks and write nothing before
  the last of them.

Recorded per call: the entry, the changed arguments (plain integers; 0 = null for a pointer; a call is a list of
numbered faults) and the return code.  The tests compare the return code and look for the entry's name at the start of
the message; the texts of two libraries are compared with --messages."""
import argparse
import base64
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "decode_refusals.json")
sys.dont_write_bytecode = True
for p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd")):
    sys.path.insert(0, p)

J, N, HH, HW, TH, TW, OH, OW, K = 17, 2, 10, 18, 5, 9, 40, 72, 30
ENTRY_BYTES = 64                                  # sizeof(SizeEntry), rtpe_decode_sizes_bytes(1)
POINTERS = ("hm", "tg", "table", "val_k", "ind_k", "tag_k", "scratch", "stream", "ans_in", "ans_out", "person_img",
            "scores", "topk_val", "topk_ind", "P_dev")


def _head(shared, sized):
    tg_planes = 1 if shared else J
    h = [("hm", 1), ("hh", HH), ("hw", HW), ("hm_img_stride", J * HH * HW), ("tg", 2), ("th", TH), ("tw", TW),
         ("tg_img_stride", tg_planes * TH * TW), ("N", N), ("J", J)]
    if sized:
        return h + [("table", 3), ("table_bytes", N * ENTRY_BYTES), ("oh", OH), ("ow", OW), ("w_enc", OW)]
    return h + [("oh", OH), ("ow", OW)]


_TOPK = [("K", K), ("nms_ksize", 5), ("nms_pad", 2), ("val_k", 4), ("ind_k", 5), ("tag_k", 6), ("scratch", 7),
         ("scratch_bytes", 1 << 30), ("stream", 0)]
_REFINE = [("ans_in", 8), ("ans_out", 9), ("person_img", 10), ("P", 0), ("do_adjust", 1), ("do_refine", 1),
           ("scores", 11)]
_TABLE = [("topk_val", 12), ("topk_ind", 13), ("K", K)]
_END = [("scratch", 7), ("scratch_bytes", 1 << 30), ("stream", 0)]

# entry -> (shared, sized, stage, argument list); stage: "topk", "refine" (no top-k table), "refine_topk", "refine_n"
ENTRIES = {}
for _suffix_topk, _names, _shared, _sized in (
        ("rtpe_topk_fused", ("rtpe_adjust_refine_fused_topk", "rtpe_adjust_refine_fused_topk_n"), False, False),
        ("rtpe_topk_fused_shared", ("rtpe_adjust_refine_fused_shared_topk", "rtpe_adjust_refine_fused_shared_topk_n"),
         True, False),
        ("rtpe_topk_fused_sizes", ("rtpe_adjust_refine_fused_topk_sizes", "rtpe_adjust_refine_fused_topk_sizes_n"),
         False, True),
        ("rtpe_topk_fused_mixed", ("rtpe_adjust_refine_fused_mixed_topk", "rtpe_adjust_refine_fused_mixed_topk_n"),
         True, True)):
    _h = _head(_shared, _sized)
    ENTRIES[_suffix_topk] = (_shared, _sized, "topk", _h + _TOPK)
    ENTRIES[_names[0]] = (_shared, _sized, "refine_topk", _h + _REFINE + _TABLE + _END)
    ENTRIES[_names[1]] = (_shared, _sized, "refine_n", _h + _REFINE + _TABLE + _END + [("P_dev", 14)])
ENTRIES["rtpe_adjust_refine_fused"] = (False, False, "refine", _head(False, False) + _REFINE + _END)


def faults(entry):
    """name -> (changed arguments, looked_at): looked_at says whether the kind's check() or the stage's own checks
    refuse the fault whatever else holds (the top-k entries need that of every call)"""
    shared, sized, stage, args = ENTRIES[entry]
    base = dict(args)
    kind = shared or sized
    f = {"hm_null": ({"hm": 0}, True), "tg_null": ({"tg": 0}, True), "N_0": ({"N": 0}, True), "J_0": ({"J": 0}, True),
         "J_33": ({"J": 33}, shared or stage != "topk"),
         "oh_0": ({"oh": 0}, kind or stage == "topk"), "ow_0": ({"ow": 0}, kind or stage == "topk")}
    for a in ("hh", "hw", "th", "tw"):
        f[a + "_0"] = ({a: 0}, kind)
    for a in ("hm_img_stride", "tg_img_stride"):
        f[a + "_short"] = ({a: base[a] - 1}, shared)
    if sized:
        f["table_null"] = ({"table": 0}, True)
        f["table_short"] = ({"table_bytes": base["table_bytes"] - 1}, True)
        f["w_enc_low"] = ({"w_enc": OW - 1}, True)
        f["index_overflow"] = ({"oh": 40000, "w_enc": 60000}, True)       # 2.4e9 > 2**31 - 1
    if stage == "topk":
        for a in ("val_k", "ind_k", "tag_k", "scratch"):
            f[a + "_null"] = ({a: 0}, True)
        f["K_0"] = ({"K": 0}, True)
        return f
    f["P_-1"] = ({"P": -1}, False)                                         # accepted, like the base call's P = 0
    f["ans_in_null"] = ({"ans_in": 0, "P": 1}, True)
    f["ans_out_null"] = ({"ans_out": 0, "P": 1}, True)
    f["ans_same"] = ({"ans_out": base["ans_in"], "P": 1}, True)
    for a in ("person_img", "scores", "scratch"):                          # not looked at before P <= 0 returns: accepted
        f[a + "_null"] = ({a: 0}, False)
    if stage != "refine":
        f["topk_val_alone"] = ({"topk_ind": 0}, True)
        f["topk_ind_alone"] = ({"topk_val": 0}, True)
        f["topk_none"] = ({"topk_val": 0, "topk_ind": 0}, True)            # these entries have no form without the table
        f["K_0"] = ({"K": 0}, True)
    if stage == "refine_n":
        f["P_dev_null"] = ({"P_dev": 0}, True)
    return f


def _arg(name, v):
    if name in POINTERS:
        return ctypes.c_void_p(v * 0x10000) if v else None
    return v


def call_entry(L, entry, changed):
    args = ENTRIES[entry][3]
    rc = getattr(L, entry)(*[_arg(n, changed.get(n, v)) for n, v in args])
    return rc, (L.rtpe_last_error_string() or b"").decode() if rc else ""


def _pairs(hw):
    return None if hw is None else (ctypes.c_int32 * (2 * len(hw)))(*[v for p in hw for v in p])


def call_fill(L, fn, c):
    """c: out_hw / heat_hw / tag_hw (lists of pairs or None), N, pitch (hh, hw, th, tw), table (bool), short (bytes the
    table is reported short by), max (bool: max_oh / max_ow asked for) -> (rc, message, table bytes, [max_oh, max_ow])"""
    n_alloc = max(c["N"], len(c["out_hw"] or []), 1)
    tab = (ctypes.c_uint8 * (n_alloc * ENTRY_BYTES))(*([0xA5] * (n_alloc * ENTRY_BYTES)))
    mh, mw = ctypes.c_int32(-1), ctypes.c_int32(-1)
    tail = (ctypes.cast(tab, ctypes.c_void_p) if c["table"] else None, c["N"] * ENTRY_BYTES - c["short"],
            ctypes.byref(mh) if c["max"] else None, ctypes.byref(mw) if c["max"] else None)
    if fn == "rtpe_decode_sizes_fill":
        rc = L.rtpe_decode_sizes_fill(_pairs(c["out_hw"]), c["N"], *c["pitch"], *tail)
    else:
        rc = L.rtpe_decode_mixed_fill(_pairs(c["out_hw"]), _pairs(c["heat_hw"]), _pairs(c["tag_hw"]), c["N"],
                                      *c["pitch"], *tail)
    msg = (L.rtpe_last_error_string() or b"").decode() if rc else ""
    return rc, msg, bytes(tab)[:max(c["N"], 0) * ENTRY_BYTES], [mh.value, mw.value]


def fill_grid():
    out, heat, tag, pitch = [[40, 72], [33, 47], [64, 20]], [[10, 18], [9, 12], [16, 5]], [[5, 9], [5, 6], [8, 3]], \
        [16, 18, 8, 9]
    base = dict(out_hw=out, heat_hw=heat, tag_hw=tag, N=3, pitch=pitch, table=True, short=0, max=True)

    def var(**kw):
        return dict(base, **kw)

    def at(lst, n, i, v):
        lst = [list(p) for p in lst]
        lst[n][i] = v
        return lst
    both = [var(), var(out_hw=None), var(table=False), var(N=0), var(short=1), var(max=False),
            var(out_hw=at(out, 1, 0, 0)), var(out_hw=at(out, 2, 1, 0)), var(out_hw=at(out, 0, 1, -3))]
    both += [var(pitch=at([pitch], 0, i, 0)[0]) for i in range(4)]
    grid = [("rtpe_decode_sizes_fill", c) for c in both] + [("rtpe_decode_mixed_fill", c) for c in both]
    mixed = [var(heat_hw=None), var(tag_hw=None)]
    for which, lst, p0 in (("heat_hw", heat, 0), ("tag_hw", tag, 2)):
        for i in (0, 1):
            mixed += [var(**{which: at(lst, 1, i, 0)}), var(**{which: at(lst, 2, i, pitch[p0 + i] + 1)}),
                      var(**{which: at(lst, 0, i, pitch[p0 + i])})]
    mixed += [var(heat_hw=at(heat, 1, 0, 0), tag_hw=None), var(out_hw=at(out, 0, 0, 0), heat_hw=at(heat, 0, 0, 17))]
    return grid + [("rtpe_decode_mixed_fill", c) for c in mixed]


def fill_shapes():
    """the four shapes whose table bytes are pinned (both fills where the shape has a meaning for both)"""
    def c(out, heat, tag, pitch):
        return dict(out_hw=out, heat_hw=heat, tag_hw=tag, N=len(out), pitch=pitch, table=True, short=0, max=True)
    one = c([[100, 140]], [[25, 35]], [[13, 18]], [27, 38, 14, 19])
    three = c([[100, 140], [33, 47], [64, 64]], [[25, 35], [9, 12], [16, 16]], [[13, 18], [5, 6], [8, 8]],
              [27, 38, 14, 19])
    full = c([[40, 72], [72, 136], [38, 58]], [[10, 18]] * 3, [[5, 9]] * 3, [10, 18, 5, 9])        # extent = pitch
    unit = c([[40, 72], [1, 1], [3, 130]], [[1, 1], [1, 18], [10, 1]], [[1, 1], [1, 1], [1, 9]], [10, 18, 5, 9])
    return [("N=1", "rtpe_decode_mixed_fill", one), ("N=1", "rtpe_decode_sizes_fill", one),
            ("N=3, mixed sizes", "rtpe_decode_mixed_fill", three), ("N=3, mixed sizes", "rtpe_decode_sizes_fill", three),
            ("extent = pitch", "rtpe_decode_mixed_fill", full), ("extent = pitch", "rtpe_decode_sizes_fill", full),
            ("extent = pitch, tag_hw null", "rtpe_decode_mixed_fill", dict(full, tag_hw=None, pitch=[10, 18, 10, 18])),
            ("extent of 1", "rtpe_decode_mixed_fill", unit)]


def entry_grid(L, entry):
    """the calls of one entry as tuples of fault names: () - the base call of an adjust + refine entry -, every fault
    alone, and every pair of faults on different arguments whose own first messages differ.  On a top-k entry a call
    without a fault that the kind looks at also holds val_k_null (see the module docstring)"""
    stage = ENTRIES[entry][2]
    fs = faults(entry)

    def call(*names):
        guarded = stage == "topk" and not any(fs[n][1] for n in names)
        return names + ("val_k_null",) if guarded else names

    def changed(names):
        return {k: v for n in names for k, v in fs[n][0].items()}
    grid = [] if stage == "topk" else [()]
    grid += [call(n) for n in fs]
    alone = {n: call_entry(L, entry, changed(call(n))) for n in fs}
    strip = lambda m: m.split(": ", 1)[-1]
    for a, b in itertools.combinations(fs, 2):
        if set(fs[a][0]) & set(fs[b][0]):
            continue
        if alone[a][0] == alone[b][0] and strip(alone[a][1]) == strip(alone[b][1]):
            continue
        grid.append(call(a, b))
    return fs, grid, changed


def record(L):
    entries = {}
    for entry, (_, _, stage, args) in ENTRIES.items():
        fs, grid, changed = entry_grid(L, entry)
        names = list(fs)
        got = {"refused": [], "accepted": []}
        for call in grid:
            rc, _ = call_entry(L, entry, changed(call))
            assert rc in (0, -1) and (rc or stage != "topk"), (entry, call, rc)    # (no sound top-k call in the grid)
            got["accepted" if rc == 0 else "refused"].append([names.index(n) for n in call])
        entries[entry] = dict(base=[[n, v] for n, v in args], faults=[[n, fs[n][0]] for n in names], **got)
    fills = [[fn, c, call_fill(L, fn, c)[0]] for fn, c in fill_grid()]
    tables = []
    for what, fn, c in fill_shapes():
        rc, _, tab, mx = call_fill(L, fn, c)
        assert rc == 0, (what, fn)
        tables.append({"shape": what, "fn": fn, "args": c, "max": mx, "table": base64.b64encode(tab).decode()})
    return {"about": "recorded by tools/gen_golden_decode_refusals.py; data only.  Per entry: the base call, the faults "
                     "(name, changed arguments; 0 = null for a pointer), and the calls as lists of fault numbers, by "
                     "return code: refused = -1, accepted = 0",
            "pointers": list(POINTERS), "entries": entries, "fills": fills, "tables": tables}


def entry_calls(fx):
    """[(entry, changed arguments, recorded return code)] of a fixture"""
    out = []
    for entry, e in fx["entries"].items():
        for rc, key in ((-1, "refused"), (0, "accepted")):
            for call in e[key]:
                out.append((entry, {k: v for i in call for k, v in e["faults"][i][1].items()}, rc))
    return out


def write(fx, path):
    """one line per entry, fill call and table: a change of the grid shows as the lines it touches"""
    d = lambda v: json.dumps(v, separators=(",", ":"))
    lines = ['{"about":%s,' % d(fx["about"]), '"pointers":%s,' % d(fx["pointers"]), '"entries":{']
    lines += ['%s:%s%s' % (d(k), d(v), "," if i + 1 < len(fx["entries"]) else "")
              for i, (k, v) in enumerate(fx["entries"].items())]
    for key in ("fills", "tables"):
        lines += ["}," if key == "fills" else "],", '"%s":[' % key]
        lines += [d(v) + ("," if i + 1 < len(fx[key]) else "") for i, v in enumerate(fx[key])]
    lines += ["]}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replay", action="store_true", help="compare the library with the file")
    ap.add_argument("--messages", metavar="FILE", help="write every call of the file with the library's answer and "
                    "message to FILE (two libraries: diff the two files)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from rtpe import _native
    L = _native.lib()
    if a.replay or a.messages:
        with open(a.out) as f:
            fx = json.load(f)
        rows = [(e, ch, rc) + call_entry(L, e, ch) for e, ch, rc in entry_calls(fx)]
        rows += [(fn, c, rc) + call_fill(L, fn, c)[:2] for fn, c, rc in fx["fills"]]
        bad = [r for r in rows if r[2] != r[3]]
        unnamed = [r for r in rows if r[3] and not r[4].startswith(r[0][len("rtpe_"):] + ":")]
        for t in fx["tables"]:
            rc, _, tab, mx = call_fill(L, t["fn"], t["args"])
            if rc or base64.b64encode(tab).decode() != t["table"] or mx != t["max"]:
                bad.append((t["fn"], t["shape"], "table bytes", rc))
        if a.messages:
            with open(a.messages, "w") as f:
                f.writelines("%s %s -> %d %s\n" % (r[0], json.dumps(r[1], sort_keys=True), r[3], r[4]) for r in rows)
        print("%s: %d calls, %d accepted, %d refused in the file; %d tables" % (
            _native.LIB_PATH, len(rows), sum(r[2] == 0 for r in rows), sum(r[2] != 0 for r in rows), len(fx["tables"])))
        print("return codes or table bytes that differ: %d; refusals that do not start with the entry's name: %d"
              % (len(bad), len(unnamed)))
        for b in bad + unnamed:
            print("  ", b)
        return 1 if bad or unnamed else 0
    fx = record(L)
    write(fx, a.out)
    n = len(entry_calls(fx))
    print("%s: %d entry calls + %d fill calls, %d tables, %d bytes" % (a.out, n, len(fx["fills"]), len(fx["tables"]),
                                                                        os.path.getsize(a.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
