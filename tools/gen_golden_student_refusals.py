#!/usr/bin/env python3
"""Generate tests/golden/student_refusals.json: the exception type and the full message of the calls that the student path
(rtpe/students.py, ``Engine._io`` / ``_io_mixed``, ``StudentPipeline``) refuses BEFORE any GPU work - and, for calls that
get through their checks on the host, what they return.  Everything runs on CPU tensors and stand-ins; no GPU is needed.

    python tools/gen_golden_student_refusals.py              # record
    python tools/gen_golden_student_refusals.py --check      # run every call of the file again and compare

The grid.  A subject is one callable with a base set of sound arguments and a list of named faults; a fault replaces one
or more arguments.  Recorded per subject: the base call, every fault alone, and every pair of faults on different
arguments whose own outcomes differ - the pair tells which of two checks comes first.  What keeps a call off the GPU:

* tensors live on the CPU (or on "meta", for "another device"), so a call that passes its checks ends at the device check
  ("HIP path only") - or, where a check behind the device check is wanted, the tensor is a CPU tensor that says
  ``is_cuda`` (``_CudaLike``) and ``CompiledModule._engine`` is replaced by a stub that raises ``AssertionError("GPU
  work")``;
* ``Engine._io`` / ``_io_mixed`` are called on a stand-in with a ``program`` and a ``device``, as the host tests do;
* ``StudentPipeline`` is made with ``__new__`` (its constructor moves the model to a GPU) around models whose forwards
  raise ``AssertionError("GPU work")``, and ``AttentionStudentStepsHalf`` itself for the model that refuses;
* ``pack_frames`` always gets ``device="cpu"``; ``stream_frames`` is called and its generator never advanced.

Only public names, the two ``Engine`` checks and the ``StudentPipeline`` methods that the host tests call are used: the
file runs unchanged before and after a refactor of the student path."""
import argparse
import itertools
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "student_refusals.json")
sys.dont_write_bytecode = True
for p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

SIZES = [(33, 47), (47, 33), (64, 32)]          # the images of every batch; their canvas is 64 x 47
OMIT = object()                                 # an argument that is not passed at all


class _CudaLike(torch.Tensor):
    """a CPU tensor that says it is on the GPU"""
    is_cuda = True


def _cuda_like(t):
    return t.as_subclass(_CudaLike)


class _NeedsAlt(torch.nn.Module):
    def forward(self, x, alt=None):
        raise AssertionError("GPU work")

    def forward_mixed(self, canvas, sizes, alt=None, att_divisor=None):
        raise AssertionError("GPU work")


class _NoAlt(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("GPU work")

    def forward_mixed(self, canvas, sizes):
        raise AssertionError("GPU work")


class _NoMixed(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("GPU work")


def _shape(v):
    if torch.is_tensor(v):
        return [str(v.dtype).replace("torch.", "")] + list(v.shape)
    if isinstance(v, (list, tuple)):
        return [_shape(t) for t in v]
    return v if isinstance(v, (int, float, str, bool, type(None))) else type(v).__name__


def subjects():
    """name -> (base arguments, {fault: replaced arguments}, call(arguments) -> something ``_shape`` can describe)"""
    import numpy as np
    from rtpe import students
    from rtpe.engine import StudentPipeline
    from rtpe.third_party.group import HeatmapParser
    from rtpe.third_party.pose_higher_hrnet import Engine
    S = {}
    g = torch.Generator().manual_seed(5)
    ims = [torch.randn(3, h, w, generator=g) for h, w in SIZES]
    alts = [torch.randn(3, h, w, generator=g) for h, w in SIZES]
    canvas, alt_canvas = torch.zeros(3, 3, 64, 47), torch.ones(3, 3, 64, 47)
    small, large, count, no_pairs = [(31, 47)] + SIZES[1:], SIZES[:2] + [(65, 32)], SIZES[:2], [1, 2, 3]
    size_faults = {"size_small": dict(sizes=small), "size_large": dict(sizes=large), "sizes_count": dict(sizes=count),
                   "sizes_no_pairs": dict(sizes=no_pairs)}

    # ---- constructors -------------------------------------------------------------------------------------------
    def ctor(cls):
        return lambda a: getattr(students, cls)(None, "cpu", **a)
    S["AttentionStudent()"] = (None, {"body_half_f32_stem": dict(body_half=True, half_precision=False)},
                               ctor("AttentionStudent"))
    S["AttentionStudentSteps()"] = (None, {"body_half": dict(body_half=True), "inplanes_50": dict(inplanes=50)},
                                    ctor("AttentionStudentSteps"))
    S["AttentionStudentStepsHalf()"] = (None, dict({"f32_stem": dict(half_precision=False), "body_half": dict(body_half=True)},
                                                   **{"inplanes_%d" % p: dict(inplanes=p) for p in (100, 50, 4, 0)}),
                                        ctor("AttentionStudentStepsHalf"))

    # ---- forward and forward_mixed of the three classes -----------------------------------------------------------
    models = {name: getattr(students, name)(None, "cpu", inplanes=48, init_fn=None).eval()
              for name in ("AttentionStudent", "AttentionStudentSteps", "AttentionStudentStepsHalf")}

    def in_mode(fn):
        def call(a):
            a = dict(a)
            model, training = a.pop("model"), a.pop("training")
            model.train(training)
            try:
                return fn(model, **{k: v for k, v in a.items() if v is not OMIT})
            finally:
                model.eval()
        return call
    x = torch.zeros(1, 3, 64, 64)
    for name, model in models.items():
        second = OMIT if name == "AttentionStudent" else torch.zeros(1, 3, 64, 64)
        faults = {"x_says_cuda": dict(x=_cuda_like(x)), "x_requires_grad": dict(x=_cuda_like(x.clone().requires_grad_())),
                  "training": dict(training=True)}
        faults.update({"alt_given": dict(alt=torch.zeros(1, 3, 64, 64))} if second is OMIT else {"alt_missing": dict(alt=None)})
        S[name + ".forward"] = (dict(model=model, training=False, x=x, alt=second), faults,
                                in_mode(lambda m, **kw: m.forward(**kw)))
        second = OMIT if name == "AttentionStudent" else alt_canvas
        faults = dict({"canvas_rank": dict(canvas=canvas[0]), "canvas_channels": dict(canvas=canvas[:, :2]),
                       "canvas_says_cuda": dict(canvas=_cuda_like(canvas)), "training": dict(training=True)}, **size_faults)
        if second is OMIT:
            faults["alt_given"] = dict(alt=alt_canvas)
        else:
            faults.update({"alt_missing": dict(alt=None), "alt_shape": dict(alt=alt_canvas[:2]),
                           "alt_width": dict(alt=alt_canvas[:, :, :, :46]), "alt_no_tensor": dict(alt=[alt_canvas]),
                           "alt_device": dict(alt=alt_canvas.to("meta"))})
        S[name + ".forward_mixed"] = (dict(model=model, training=False, canvas=canvas, sizes=SIZES, alt=second), faults,
                                      in_mode(lambda m, **kw: m.forward_mixed(**kw)))

    # ---- Engine._io / _io_mixed on a stand-in ---------------------------------------------------------------------
    prog = lambda **kw: types.SimpleNamespace(**kw)
    any_size = prog(any_size=True, has_aux=False, outputs=[(1, 2), (18, 2)])
    with_aux = prog(any_size=True, has_aux=True, outputs=[(1, 2), (18, 2)])
    teacher = prog(any_size=False, has_aux=False, outputs=[(34, 2), (17, 1)])
    cpu, gpu = torch.device("cpu"), torch.device("cuda", 0)
    xb = torch.zeros(2, 3, 64, 96)

    def io(a):
        r = Engine._io(types.SimpleNamespace(program=a["program"], device=a["device"]), a["x"], a["out_dtype"])
        return list(r[1:4]) + [_shape(r[4]), _shape(r[5]), r[6], r[7], r[0].is_contiguous()]
    S["Engine._io"] = (
        dict(program=any_size, device=cpu, x=_cuda_like(xb), out_dtype=torch.float32),
        {"rank": dict(x=_cuda_like(xb[0])), "channels": dict(x=_cuda_like(xb[:, :2])), "dtype": dict(x=_cuda_like(xb.double())),
         "on_cpu": dict(x=xb), "other_device": dict(device=gpu), "side_small": dict(x=_cuda_like(xb[:, :, :31])),
         "ragged": dict(x=_cuda_like(xb[:, :, :33, :47])), "teacher": dict(program=teacher),
         "half": dict(x=_cuda_like(xb.half())), "out_half": dict(out_dtype=torch.float16),
         "strided": dict(x=_cuda_like(torch.zeros(2, 64, 96, 3).permute(0, 3, 1, 2)))}, io)

    def io_mixed(a):
        r = Engine._io_mixed(types.SimpleNamespace(program=a["program"], device=a["device"]), a["x"], a["sizes"], a["aux"])
        return [len(r), r[0].is_contiguous()] + list(r[1:5]) + [_shape(t) for t in r[5:]]
    io_mixed_faults = dict({"teacher": dict(program=teacher), "rank": dict(x=_cuda_like(canvas[0])),
                            "channels": dict(x=_cuda_like(canvas[:, :2])), "dtype": dict(x=_cuda_like(canvas.double())),
                            "on_cpu": dict(x=canvas), "other_device": dict(device=gpu), "half": dict(x=_cuda_like(canvas.half()))},
                           **size_faults)
    S["Engine._io_mixed"] = (dict(program=any_size, device=cpu, x=_cuda_like(canvas), sizes=SIZES, aux=None),
                             dict(io_mixed_faults, aux_given=dict(aux=alt_canvas)), io_mixed)
    S["Engine._io_mixed, second input"] = (
        dict(program=with_aux, device=cpu, x=_cuda_like(canvas), sizes=SIZES, aux=alt_canvas),
        dict(io_mixed_faults, aux_missing=dict(aux=None), aux_shape=dict(aux=alt_canvas[:2]),
             aux_height=dict(aux=alt_canvas[:, :, :63]), aux_double=dict(aux=alt_canvas.double()),
             aux_half=dict(aux=alt_canvas.half()), aux_device=dict(aux=alt_canvas.to("meta")),
             no_second_input=dict(program=any_size)), io_mixed)

    # ---- StudentPipeline ------------------------------------------------------------------------------------------
    def pipe(model):
        p = StudentPipeline.__new__(StudentPipeline)
        p.model, p.parser = model, HeatmapParser(17, 30, 0.1, 1.0, True, False)
        p.flip_test, p.scale_factors, p.ags = False, None, False
        p.device = torch.device("cpu")
        return p
    refuses = models["AttentionStudentStepsHalf"]
    kinds = {"second input": (_NeedsAlt(), _NoAlt()), "no second input": (_NoAlt(), _NeedsAlt())}
    one_small = [torch.zeros(3, 31, 40)] + ims[1:]

    def model_faults(other):
        return {"model_without_forward_mixed": dict(model=_NoMixed()), "model_refuses": dict(model=refuses),
                "model_of_the_other_kind": dict(model=other)}
    forms = {"images": lambda a: a["images"], "(images, alts)": lambda a: (a["images"], a["alts"]),
             "(canvas, sizes)": lambda a: (a["canvas"], a["sizes"]),
             "(canvas, sizes, alt)": lambda a: (a["canvas"], a["sizes"], a["alt"])}
    image_faults = {"image_small": dict(images=one_small), "image_rank": dict(images=[ims[0], ims[1][0], ims[2]]),
                    "image_device": dict(images=[ims[0], ims[1].to("meta"), ims[2]]), "no_images": dict(images=[]),
                    "one_tensor": dict(images=canvas)}
    alts_faults = {"alts_count": dict(alts=alts[:2]), "alt_size": dict(alts=[alts[0], alts[0], alts[2]]),
                   "alt_rank": dict(alts=[alts[0][None], alts[1], alts[2]]), "alts_none": dict(alts=None),
                   "alt_no_tensor": dict(alts=[alts[0], None, alts[2]])}
    canvas_faults = dict({"canvas_rank": dict(canvas=canvas[0]), "canvas_channels": dict(canvas=canvas[:, :2]),
                          "canvas_no_tensor": dict(canvas=[canvas]), "sizes_none": dict(sizes=None)}, **size_faults)
    alt_canvas_faults = {"alt_shape": dict(alt=alt_canvas[:2]), "alt_width": dict(alt=alt_canvas[:, :, :, :40]),
                         "alt_device": dict(alt=alt_canvas.to("meta")), "alt_no_tensor": dict(alt=[alt_canvas]),
                         "alt_none": dict(alt=None)}
    for kind, (model, other) in kinds.items():
        for form, batch_of in forms.items():
            faults = model_faults(other)
            faults.update(image_faults if "images" in form else canvas_faults)
            faults.update(alts_faults if "alts" in form else alt_canvas_faults if "alt" in form else {})

            def begin(a, batch_of=batch_of):
                batch, hw = pipe(a["model"])._mixed_begin(batch_of(a))
                return [_shape(list(batch)), hw]
            S["_mixed_begin, %s, %s" % (kind, form)] = (
                dict(model=model, images=ims, alts=alts, canvas=canvas, sizes=SIZES, alt=alt_canvas), faults, begin)
        given = kind == "second input"
        call_faults = dict(model_faults(other), decode_unknown=dict(decode="image"), decode_per_image=dict(decode="per_image"),
                           ids_count=dict(image_ids=[1, 2]), ids_given=dict(image_ids=[1, 2, 3]))
        S["call_mixed, %s" % kind] = (
            dict(model=model, images=ims, image_ids=None, decode="batch", alt=alts if given else None),
            dict(call_faults, **image_faults, **({"alts_count": dict(alt=alts[:2]), "alt_size": dict(alt=[alts[0], alts[0], alts[2]]),
                                                  "alt_rank": dict(alt=[alts[0][None], alts[1], alts[2]]),
                                                  "alt_missing": dict(alt=None)} if given else {"alt_given": dict(alt=alts)})),
            lambda a: pipe(a["model"]).call_mixed(a["images"], a["image_ids"], a["decode"], a["alt"]))
        frames = [np.zeros((h, w, 3), np.uint8) for h, w in SIZES]
        frame_faults = {"no_frames": dict(frames=[]), "frame_float": dict(frames=[frames[0], frames[1].astype(np.float32)]),
                        "frame_small": dict(frames=[frames[0], np.zeros((31, 40, 3), np.uint8)]),
                        "one_3d_array": dict(frames=frames[0]), "colorspace_unknown": dict(alt_colorspace="XYZ"),
                        ("colorspace_missing" if given else "colorspace_given"): dict(alt_colorspace=None if given else "LAB")}
        S["call_frames, %s" % kind] = (
            dict(model=model, frames=frames, alt_colorspace="LAB" if given else None, image_ids=None, decode="batch"),
            dict(call_faults, **frame_faults),
            lambda a: pipe(a["model"]).call_frames(a["frames"], a["alt_colorspace"], a["image_ids"], a["decode"]))
        S["stream_frames, %s" % kind] = (
            dict(model=model, frames=frames, alt_colorspace="LAB" if given else None),
            dict(model_faults(other), **frame_faults),
            lambda a: type(pipe(a["model"]).stream_frames([a["frames"]], a["alt_colorspace"])).__name__)
    shapes = [types.SimpleNamespace(shape=(3, h, w)) for h, w in SIZES + [(40, 40), (90, 35)]]
    cut_faults = {"batch_size_0": dict(batch_size=0), "batch_size_negative": dict(batch_size=-2), "alts_count": dict(alts=shapes[:4])}
    S["mixed_batches"] = (dict(images=shapes, batch_size=2, alts=shapes), cut_faults,
                          lambda a: [[len(b[0]), len(b[1])] for b in
                                     StudentPipeline.mixed_batches(a["images"], a["batch_size"], a["alts"])[0]])
    S["frame_batches"] = (dict(images=[types.SimpleNamespace(shape=(h, w, 3)) for h, w in SIZES], batch_size=2),
                          {k: v for k, v in cut_faults.items() if "alts" not in k},
                          lambda a: [len(b) for b in StudentPipeline.frame_batches(a["images"], a["batch_size"])[0]])

    # ---- pack_mixed / pack_frames ---------------------------------------------------------------------------------
    def packed(a):
        c, sizes = students.pack_mixed(a["images"], a["canvas_hw"])
        return [_shape(c), sizes]
    S["pack_mixed"] = (
        dict(images=ims, canvas_hw=None),
        dict({k: v for k, v in image_faults.items() if k != "one_tensor"},
             image_no_tensor=dict(images=[ims[0], ims[1].numpy(), ims[2]]), image_channels=dict(images=[ims[0], ims[1][:2], ims[2]]),
             canvas_low=dict(canvas_hw=(63, 47)), canvas_narrow=dict(canvas_hw=(64, 46)), canvas_larger=dict(canvas_hw=(72, 80))),
        packed)
    frames = [np.zeros((h, w, 3), np.uint8) for h, w in SIZES]
    out = (torch.zeros(3, 3, 64, 47), torch.zeros(3, 3, 64, 47))
    S["pack_frames"] = (
        dict(frames=frames, alt_colorspace="LAB", canvas_hw=None, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), out=out),
        {"no_frames": dict(frames=[]), "one_3d_array": dict(frames=frames[0]), "one_3d_tensor": dict(frames=torch.zeros(33, 47, 3)),
         "one_4d_array": dict(frames=np.zeros((3, 64, 47, 3), np.uint8)), "colorspace_unknown": dict(alt_colorspace="XYZ"),
         "frame_float": dict(frames=[frames[0], frames[1].astype(np.float32), frames[2]]),
         "frame_channels": dict(frames=[frames[0], np.zeros((47, 33, 4), np.uint8), frames[2]]),
         "frame_rank": dict(frames=[frames[0], frames[1][0], frames[2]]), "frame_list": dict(frames=[frames[0], [1, 2], frames[2]]),
         "frame_small": dict(frames=[frames[0], np.zeros((31, 40, 3), np.uint8), frames[2]]),
         "canvas_low": dict(canvas_hw=(63, 47)), "std_zero": dict(std=(0.25, 0.0, 0.25)), "mean_two": dict(mean=(0.5, 0.5)),
         "out_one": dict(out=(out[0],)), "out_no_tuple": dict(out=out[0]), "out_without_alt": dict(out=(out[0], None)),
         "no_colorspace": dict(alt_colorspace=None), "out_shape": dict(out=(out[0], out[1][:2])),
         "out_first_shape": dict(out=(out[0][:, :, :63], out[1])), "out_double": dict(out=(out[0], out[1].double())),
         "out_strided": dict(out=(out[0], torch.zeros(3, 3, 47, 64).transpose(2, 3))),
         "out_device": dict(out=(out[0], out[1].to("meta"))), "out_no_tensor": dict(out=(out[0], "alt")), "out_none": dict(out=None)},
        lambda a: _shape(list(students.pack_frames(a["frames"], a["alt_colorspace"], a["canvas_hw"], a["mean"], a["std"],
                                                   "cpu", a["out"]))))
    return S


def outcome(subject, names):
    """[exception type, message] of the subject's call with the named faults, or ["returned", description]"""
    base, faults, call = subject
    args = dict(base or {})
    for n in names:
        args.update(faults[n])
    try:
        return ["returned", json.loads(json.dumps(_shape(call(args))))]
    except Exception as e:                      # (every kind: the type is what is recorded)
        return [type(e).__name__, str(e)]


def no_gpu():
    """``CompiledModule._engine`` replaced by a stub for the time of a run; returns the function that puts it back"""
    from rtpe.third_party.pose_higher_hrnet import CompiledModule
    real = CompiledModule._engine

    def stub(self, *a, **k):
        raise AssertionError("GPU work")
    CompiledModule._engine = stub
    return lambda: setattr(CompiledModule, "_engine", real)


def grid(subject):
    """the calls of one subject as tuples of fault names: the base call where there is one, every fault alone, every
    pair of faults on different arguments whose own outcomes differ"""
    base, faults, _ = subject
    calls = ([()] if base is not None else []) + [(n,) for n in faults]
    alone = {n: outcome(subject, (n,)) for n in faults}
    for a, b in itertools.combinations(faults, 2):
        if not set(faults[a]) & set(faults[b]) and alone[a] != alone[b]:
            calls.append((a, b))
    return calls


def record():
    restore = no_gpu()
    try:
        outcomes, out = [], {}
        for name, subject in subjects().items():
            names = list(subject[1])
            calls = []
            for call in grid(subject):
                o = outcome(subject, call)
                if o not in outcomes:
                    outcomes.append(o)
                calls.append([[names.index(n) for n in call], outcomes.index(o)])
            out[name] = {"faults": names, "calls": calls}
    finally:
        restore()
    return {"about": "recorded by tools/gen_golden_student_refusals.py; data only.  outcomes: [exception type, message] or "
                     "[\"returned\", description], each once; per subject the names of its faults and its calls as [[fault "
                     "numbers], outcome number] - no fault: the base call",
            "outcomes": outcomes, "subjects": out}


def replay(fx):
    """every call of a fixture run again -> [(subject, fault names, recorded outcome, outcome now)]"""
    restore = no_gpu()
    try:
        have = subjects()
        rows = []
        for name, s in fx["subjects"].items():
            for call, o in s["calls"]:
                names = tuple(s["faults"][i] for i in call)
                known = name in have and all(n in have[name][1] for n in names)
                rows.append((name, names, fx["outcomes"][o], outcome(have[name], names) if known else ["missing", ""]))
    finally:
        restore()
    return rows


def write(fx, path):
    """one line per outcome and per subject: a change shows as the lines it touches"""
    d = lambda v: json.dumps(v, separators=(",", ":"))
    lines = ['{"about":%s,' % d(fx["about"]), '"outcomes":[']
    lines += [d(o) + ("," if i + 1 < len(fx["outcomes"]) else "") for i, o in enumerate(fx["outcomes"])]
    lines += ['],', '"subjects":{']
    lines += ['%s:%s%s' % (d(k), d(v), "," if i + 1 < len(fx["subjects"]) else "")
              for i, (k, v) in enumerate(fx["subjects"].items())]
    lines += ["}}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="run every call of the file again and compare")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.check:
        with open(a.out) as f:
            fx = json.load(f)
        rows = replay(fx)
        bad = [r for r in rows if r[2] != r[3]]
        print("%s: %d calls of %d subjects, %d refused, %d returned; %d differ" % (
            a.out, len(rows), len(fx["subjects"]), sum(r[2][0] != "returned" for r in rows),
            sum(r[2][0] == "returned" for r in rows), len(bad)))
        for name, names, want, got in bad:
            print("  %s %s\n    recorded: %s\n    now:      %s" % (name, list(names), want, got))
        return 1 if bad else 0
    fx = record()
    write(fx, a.out)
    n = sum(len(s["calls"]) for s in fx["subjects"].values())
    print("%s: %d calls of %d subjects, %d distinct outcomes, %d bytes" % (a.out, n, len(fx["subjects"]), len(fx["outcomes"]),
                                                                           os.path.getsize(a.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
