"""CPU tests of the student path as a whole (rtpe/students.py, ``Engine``'s call preparation, ``StudentPipeline``'s batch
checks): what the three classes register and compile, and what every host-side check refuses, are what they were at the
commit the two fixtures were recorded from.  The fixtures are data only; the tools that wrote them
(tools/gen_golden_student_programs.py, tools/gen_golden_student_refusals.py: the case matrix, the grid of faults and what
keeps every call off the GPU) compute the same things again here."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_student_programs_are_what_the_parent_compiled(golden_dir):
    """the ordered state-dict keys of every case and, per compiled program, the SHA-256 over ops, tensors and weight blob,
    the op names, the outputs and the two program properties"""
    tool = _tool("gen_golden_student_programs")
    with open(os.path.join(golden_dir, "student_program_digests.json")) as f:
        want = json.load(f)
    assert len(want["cases"]) == len(tool.CASES) == 13 and tool.n_programs(want) == 22
    got = json.loads(json.dumps(tool.record()))
    assert tool.differences(want, got) == []
    assert got["cases"] == want["cases"] and got["key_lists"] == want["key_lists"]


def test_student_refusals_are_the_parents(golden_dir):
    """exception type and full message of every recorded call - each fault alone and every pair of faults whose own
    outcomes differ, which pins the order of the checks - and the description of what the accepted calls return"""
    tool = _tool("gen_golden_student_refusals")
    with open(os.path.join(golden_dir, "student_refusals.json")) as f:
        want = json.load(f)
    rows = tool.replay(want)
    assert len(rows) == 1588 and len(want["subjects"]) == 30
    bad = [r for r in rows if r[2] != r[3]]
    assert not bad, "%d of %d calls differ, the first: %s" % (len(bad), len(rows), bad[0])
