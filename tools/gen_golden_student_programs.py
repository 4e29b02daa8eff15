#!/usr/bin/env python3
"""Generate tests/golden/student_program_digests.json: what the three student classes of rtpe/students.py register and
compile, recorded so that a change of the Python that builds them (constructors, ``ContextAwareModule.emit``, the
``compile_program`` recipes) can be told from a change of what they build.  No GPU is needed: a program is compiled on
the host.

    python tools/gen_golden_student_programs.py            # record
    python tools/gen_golden_student_programs.py --check    # recompute and compare with the file

Per case: the ordered ``state_dict()`` keys (stored once per distinct list), and per compiled program a SHA-256 over
``bytes(program.ops)``, ``bytes(program.tensors)`` and ``program.blob``, with ``program.names``, ``program.outputs``,
``any_size`` and ``has_aux``.

The cases.  "init": ``torch.manual_seed(0)`` and the constructor's default ``init_fn`` - the digest then pins the order in
which the modules are registered and in which the initialiser draws.  "synth": ``init_fn=None`` and the seeded W1
weights of ``oracle.synth.make_state_dict`` over the shapes of tests/golden/student*_shapes.json - BatchNorm statistics
that are not the identity, so the folded (alpha, beta) are pinned too.  The Steps classes compile one program per
``att_divisor``: None and 20.0.

The digests are the same on every host: the one host-dependent step of a compile, the float32 ``torch.sqrt`` in the fold of
a BatchNorm, is taken in float64 and rounded once while the tool compiles (``sqrt_rounded_once``).

Only public names are used: the file runs unchanged before and after a refactor of the students."""
import argparse
import contextlib
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "student_program_digests.json")
sys.dont_write_bytecode = True
for p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd")):
    sys.path.insert(0, p)

DIVISORS = (None, 20.0)
# name, class, constructor keywords, weights: "init" or (shapes file, seed)
CASES = (
    ("student48", "AttentionStudent", dict(inplanes=48), "init"),
    ("student104_body_half", "AttentionStudent", dict(inplanes=104, body_half=True), "init"),
    ("student64_f32_stem", "AttentionStudent", dict(inplanes=64, half_precision=False), "init"),
    ("steps48", "AttentionStudentSteps", dict(inplanes=48), "init"),
    ("steps80", "AttentionStudentSteps", dict(inplanes=80), "init"),
    ("steps48_f32_stem", "AttentionStudentSteps", dict(inplanes=48, half_precision=False), "init"),
    ("steps_half48", "AttentionStudentStepsHalf", dict(inplanes=48), "init"),
    ("steps_half80", "AttentionStudentStepsHalf", dict(inplanes=80), "init"),
    ("student100_synth", "AttentionStudent", dict(inplanes=100), ("student_shapes.json", 3)),
    ("steps48_synth", "AttentionStudentSteps", dict(inplanes=48), ("student_steps_shapes.json", 4)),
    ("steps80_synth", "AttentionStudentSteps", dict(inplanes=80), ("student_steps80_shapes.json", 4)),
    ("steps_half48_synth", "AttentionStudentStepsHalf", dict(inplanes=48), ("student_steps_shapes.json", 4)),
    ("steps_half80_synth", "AttentionStudentStepsHalf", dict(inplanes=80), ("student_steps80_shapes.json", 4)),
)


def build_model(cls_name, kwargs, weights):
    import torch
    from oracle import synth
    from rtpe import students
    cls = getattr(students, cls_name)
    if weights == "init":
        torch.manual_seed(0)
        return cls(None, "cpu", **kwargs).eval()
    shapes_file, seed = weights
    with open(os.path.join(GOLDEN, shapes_file)) as f:
        shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
    model = cls(None, "cpu", init_fn=None, **kwargs).eval()
    model.load_state_dict(synth.make_state_dict(shapes, seed, "W1"), strict=True)
    return model


def describe(program):
    h = hashlib.sha256()
    for part in (bytes(program.ops), bytes(program.tensors), program.blob):
        h.update(part)
    return {"sha256": h.hexdigest(), "names": list(program.names), "outputs": [list(o) for o in program.outputs],
            "any_size": bool(program.any_size), "has_aux": bool(program.has_aux)}


@contextlib.contextmanager
def sqrt_rounded_once():
    """``torch.sqrt`` of a float32 tensor on the CPU goes through a vendor math library whose last bit depends on the host's
    CPU model (seen: two AVX-512 machines, the same torch build, other bits), and the fold of a BatchNorm
    (``1 / sqrt(var + eps)``) calls it - with statistics that are not the identity the weight blob then differs from host to
    host.  While a program is compiled for its digest the root is taken in float64 and rounded once, which every host
    does alike; everything else of the fold is the code's own."""
    import torch
    real = torch.sqrt
    torch.sqrt = lambda t: real(t.double()).to(t.dtype)
    try:
        yield
    finally:
        torch.sqrt = real


def record():
    with sqrt_rounded_once():
        return _record()


def _record():
    key_lists, cases = [], {}
    for name, cls_name, kwargs, weights in CASES:
        model = build_model(cls_name, kwargs, weights)
        keys = list(model.state_dict().keys())
        if keys not in key_lists:
            key_lists.append(keys)
        if cls_name == "AttentionStudent":
            programs = {"plain": describe(model.compile_program())}
        else:
            programs = {"att_divisor=%s" % d: describe(model.compile_program(("att_divisor", d))) for d in DIVISORS}
        cases[name] = {"class": cls_name, "kwargs": kwargs, "weights": weights if weights == "init" else list(weights),
                       "keys": key_lists.index(keys), "programs": programs}
    return {"about": "recorded by tools/gen_golden_student_programs.py; data only.  Per case: the index of its ordered "
                     "state_dict() keys in key_lists, and per compiled program the SHA-256 over ops, tensors and weight "
                     "blob, the op names, the outputs (channels, log2 down-scale) and the two program properties",
            "key_lists": key_lists, "cases": cases}


def differences(want, got):
    """what differs between two fixtures, one line each"""
    out = []
    for name, w in want["cases"].items():
        g = got["cases"].get(name)
        if g is None:
            out.append("%s: not computed" % name)
            continue
        if want["key_lists"][w["keys"]] != got["key_lists"][g["keys"]]:
            out.append("%s: state_dict() keys or their order" % name)
        for variant, wp in w["programs"].items():
            gp = g["programs"].get(variant, {})
            out += ["%s %s: %s" % (name, variant, field) for field in wp if wp[field] != gp.get(field)]
    return out + ["%s: not in the file" % n for n in got["cases"] if n not in want["cases"]]


def n_programs(fx):
    return sum(len(c["programs"]) for c in fx["cases"].values())


def write(fx, path):
    """one line per key list and per case: a change shows as the lines it touches"""
    d = lambda v: json.dumps(v, separators=(",", ":"))
    lines = ['{"about":%s,' % d(fx["about"]), '"key_lists":[']
    lines += [d(k) + ("," if i + 1 < len(fx["key_lists"]) else "") for i, k in enumerate(fx["key_lists"])]
    lines += ['],', '"cases":{']
    lines += ['%s:%s%s' % (d(k), d(v), "," if i + 1 < len(fx["cases"]) else "") for i, (k, v) in enumerate(fx["cases"].items())]
    lines += ["}}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="recompute and compare with the file")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    fx = record()
    if a.check:
        with open(a.out) as f:
            want = json.load(f)
        bad = differences(want, json.loads(json.dumps(fx)))
        print("%s: %d cases, %d programs; %d differences" % (a.out, len(want["cases"]), n_programs(want), len(bad)))
        for b in bad:
            print("  ", b)
        return 1 if bad else 0
    write(fx, a.out)
    print("%s: %d cases, %d programs, %d key lists, %d bytes" % (a.out, len(fx["cases"]), n_programs(fx),
                                                                 len(fx["key_lists"]), os.path.getsize(a.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
