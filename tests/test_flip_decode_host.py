"""CPU tests of the batched flip-test decode: the host-side grouping of images by network input size, the ABI of the
new entries, and the compiled flip decode kernels (no registers spilled to scratch memory)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


def _device_code(built, tmp_path, name):
    """disassembly of the gfx950 code object inside build/<name>.o (a copy: the test must not touch build products)"""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin/"
    obj = shutil.copy(os.path.join(os.path.dirname(built.LIB_PATH), "build", name + ".o"), str(tmp_path / (name + ".o")))
    fat, co = str(tmp_path / (name + ".fatbin")), str(tmp_path / (name + ".co"))
    subprocess.run([llvm + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj, str(tmp_path / (name + ".2.o"))], check=True)
    subprocess.run([llvm + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + co], check=True)
    return subprocess.run([llvm + "llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout


def test_group_by_input_size_keeps_the_input_order():
    from rtpe.inference import group_by_input_size
    from rtpe.third_party import transforms
    shapes = [(427, 640), (640, 480), (640, 640), (427, 640), (640, 640), (640, 480), (427, 640)]
    sizes = [transforms.get_multi_scale_size(np.zeros(s + (3,), np.uint8), 640, 1.0, 1)[0] for s in shapes]
    assert sizes[0] == (960, 640) and sizes[1] == (640, 896) and sizes[2] == (640, 640)
    groups = group_by_input_size(sizes)
    assert groups == [((960, 640), [0, 3, 6]), ((640, 896), [1, 5]), ((640, 640), [2, 4])]
    assert group_by_input_size([]) == []


NEW_SYMBOLS = ("rtpe_flip_maps_bytes", "rtpe_topk_flip", "rtpe_adjust_refine_flip")


def test_flip_symbols_are_declared_and_resolve(built):
    hdr = open(os.path.join(ROOT, "include", "rtpe_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", hdr))
    lib = built.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in built.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.rtpe_version() == 4


def test_flip_maps_bytes(built):
    import ctypes
    nb = ctypes.c_size_t()
    built.check(built.lib().rtpe_flip_maps_bytes(32, 17, 320, 320, ctypes.byref(nb)))
    assert nb.value == 4 * 32 * 17 * 320 * 320 * 4
    with pytest.raises(RuntimeError):
        built.check(built.lib().rtpe_flip_maps_bytes(0, 17, 320, 320, ctypes.byref(nb)))


def test_flip_decode_kernels_do_not_spill(built, tmp_path):
    dis = _device_code(built, tmp_path, "decode.hip")
    bodies = re.split(r"\n(?=[0-9a-f]+ <)", dis)
    flip = [b for b in bodies if re.match(r"[0-9a-f]+ <\S*(FlipHeatMap|FlipTag|flip_prep_kernel)", b)]
    names = [b.split("<", 1)[1].split(">", 1)[0] for b in flip]
    assert any("flip_prep_kernel" in n for n in names)
    assert any("topk_tile_kernel" in n for n in names) and any("topk_merge_kernel" in n for n in names)
    assert any("refine_scan_kernel" in n for n in names)
    for n, b in zip(names, flip):
        assert "scratch_" not in b, n + ": registers spilled to scratch memory"
