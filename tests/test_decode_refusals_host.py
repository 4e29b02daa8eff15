"""CPU tests of what the network-output decode entries of csrc/decode.hip (plain, `_shared`, `_sizes`, `_mixed`: top-k,
adjust + refine, `_n`) and the two size-table fills answer before any launch: tests/golden/decode_refusals.json holds a
grid of calls, each with the return code it got when the four kinds were four structs
(tools/gen_golden_decode_refusals.py: which calls, and why none of them reaches memory or the GPU), and the bytes the
fills wrote on four shapes.  The library of the tree must answer every call alike and name the entry that was called at
the start of every refusal."""
import base64
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_BYTES = 64


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "decode_refusals.json")) as f:
        return json.load(f)


def _message(L, rc):
    return (L.rtpe_last_error_string() or b"").decode() if rc else ""


def _calls(fx):
    """[(entry, changed arguments, recorded return code)]: a recorded call is a list of the entry's numbered faults"""
    out = []
    for entry, e in fx["entries"].items():
        for want, key in ((-1, "refused"), (0, "accepted")):
            out += [(entry, {k: v for i in call for k, v in e["faults"][i][1].items()}, want) for call in e[key]]
    return out


def _call_entry(L, fx, entry, changed):
    pointers = set(fx["pointers"])
    args = []
    for name, v in fx["entries"][entry]["base"]:
        v = changed.get(name, v)
        args.append((ctypes.c_void_p(v * 0x10000) if v else None) if name in pointers else v)     # fake addresses
    rc = getattr(L, entry)(*args)
    return rc, _message(L, rc)


def _pairs(hw):
    return None if hw is None else (ctypes.c_int32 * (2 * len(hw)))(*[v for p in hw for v in p])


def _call_fill(L, fn, c):
    """the generator's call_fill: real arrays, a real table pre-set to 0xA5 -> (rc, message, table bytes, [max_oh, max_ow])"""
    n_alloc = max(c["N"], len(c["out_hw"] or []), 1)
    tab = (ctypes.c_uint8 * (n_alloc * ENTRY_BYTES))(*([0xA5] * (n_alloc * ENTRY_BYTES)))
    mh, mw = ctypes.c_int32(-1), ctypes.c_int32(-1)
    tail = (ctypes.cast(tab, ctypes.c_void_p) if c["table"] else None, c["N"] * ENTRY_BYTES - c["short"],
            ctypes.byref(mh) if c["max"] else None, ctypes.byref(mw) if c["max"] else None)
    if fn == "rtpe_decode_sizes_fill":
        rc = L.rtpe_decode_sizes_fill(_pairs(c["out_hw"]), c["N"], *c["pitch"], *tail)
    else:
        rc = L.rtpe_decode_mixed_fill(_pairs(c["out_hw"]), _pairs(c["heat_hw"]), _pairs(c["tag_hw"]), c["N"], *c["pitch"],
                                      *tail)
    return rc, _message(L, rc), bytes(tab)[:max(c["N"], 0) * ENTRY_BYTES], [mh.value, mw.value]


def test_the_fixture_covers_the_thirteen_entries_and_both_fills(built, fx):
    calls = _calls(fx)
    entries = {c[0] for c in calls}
    assert entries == set(fx["entries"]) and len(entries) == 13
    known = set(built.EXPORTS) | set(built.EXPORTS_SHARED) | set(built.EXPORTS_SIZES) | set(built.EXPORTS_MIXDEC)
    assert entries <= known
    assert {c[0] for c in fx["fills"]} == {"rtpe_decode_sizes_fill", "rtpe_decode_mixed_fill"}
    # the only accepted adjust + refine calls are those for nobody; no top-k call of the grid is accepted
    for entry, changed, rc in calls:
        if rc == 0:
            assert "adjust_refine" in entry and changed.get("P", 0) <= 0, (entry, changed)
    assert len(calls) > 2000 and sum(c[2] == 0 for c in calls) >= 13


def test_every_recorded_call_gets_the_recorded_answer_and_a_refusal_names_its_entry(built, fx):
    L = built.lib()
    for entry, changed, want in _calls(fx):
        rc, msg = _call_entry(L, fx, entry, changed)
        assert rc == want, (entry, changed, msg)
        if rc:
            assert msg.startswith(entry[len("rtpe_"):] + ":"), (entry, changed, msg)
    for fn, c, want in fx["fills"]:
        rc, msg, _, _ = _call_fill(L, fn, c)
        assert rc == want, (fn, c, msg)
        if rc:
            assert msg.startswith(fn[len("rtpe_"):] + ":"), (fn, c, msg)


def test_refusal_texts_that_other_tests_and_callers_look_for(built, fx):
    L = built.lib()
    seen = {}
    for entry, changed, want in _calls(fx):
        if want:
            seen.setdefault(tuple(sorted(changed.items())), {})[entry] = _call_entry(L, fx, entry, changed)[1]
    for entry in fx["entries"]:
        if entry.endswith("_n"):
            assert "P_dev is null" in seen[(("P_dev", 0),)][entry]
        if "shared" in entry or "mixed" in entry:
            assert "J <= 32" in seen[(("J", 33),)][entry]
            assert "image stride" in seen[(("tg_img_stride", dict(fx["entries"][entry]["base"])["tg_img_stride"] - 1),)][entry]
        if "sizes" in entry or "mixed" in entry:
            assert "w_enc=71" in seen[(("w_enc", 71),)][entry] and "table too small" in \
                seen[(("table_bytes", 127),)][entry]


SHAPES = ["N=1", "N=3, mixed sizes", "extent = pitch", "extent of 1"]


@pytest.mark.parametrize("shape", SHAPES)
def test_the_fills_write_the_recorded_table_bytes(built, fx, shape):
    L = built.lib()
    cases = [t for t in fx["tables"] if t["shape"].startswith(shape)]
    assert cases and {t["shape"].split(",")[0] for t in fx["tables"]} == {s.split(",")[0] for s in SHAPES}
    for t in cases:
        rc, msg, tab, mx = _call_fill(L, t["fn"], t["args"])
        assert rc == 0, msg
        assert tab == base64.b64decode(t["table"]) and len(tab) == t["args"]["N"] * ENTRY_BYTES, (t["fn"], t["shape"])
        assert mx == t["max"] == [max(p[i] for p in t["args"]["out_hw"]) for i in (0, 1)]
    if shape == "extent = pitch":       # the sizes fill is the mixed fill with every extent equal to its pitch
        both = {t["fn"]: t["table"] for t in cases if t["shape"] == shape}
        assert len(both) == 2 and len(set(both.values())) == 1
