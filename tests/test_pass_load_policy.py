"""The load policy of the IRLS passes in the BUILT product library (sf_irls.h: pass_division): each pass
has two instances of its streaming loop, one whose eight record loads are all non-temporal (`global_load_* ... nt`) and one whose
loads are all default-policy (the window the next pass starts on). The compiler drops the nt bit when it merges an nt load with a
plain one, so the property is checked where it shows: the disassembly (tools/diag/loop_waits.py), for every build of the frame
kernel the library holds. Both instances keep the shape the passes rely on: the record of the next trip in flight during the
current one (the waits for it stand at the end of the trip and end in vmcnt(2), vmcnt(0)) and no scratch access inside a loop."""
import functools
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ("irls_pass1ILi0", "irls_pass2ILi0ELi0", "irls_pass2ILi0ELi1")  # the product's pass 1, pass 2 upwards, pass 2 back down


@functools.lru_cache(maxsize=None)
def _loop_waits():
    spec = importlib.util.spec_from_file_location("loop_waits", os.path.join(ROOT, "tools", "diag", "loop_waits.py"))
    lw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lw)
    lw.exec_lint.code_objects = functools.lru_cache(maxsize=None)(lw.exec_lint.code_objects)  # disassemble the library once
    return lw


@pytest.mark.parametrize("kern", ["256", "256o5", "1024", "cluster"])
def test_each_pass_has_one_nt_loop_and_one_default_loop(kern):
    lw = _loop_waits()
    if not os.path.exists(lw.exec_lint.OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    lib = os.path.join(ROOT, "staticfusion_amd", "csrc", "libsf_hip.so")
    for fn in PASSES:
        streaming = [r for r in lw.innermost_loops(lib, kern, fn) if r["loads"]]
        assert len(streaming) == 2, (kern, fn, streaming)
        assert sorted(r["nt_loads"] for r in streaming) == [0, 8], (kern, fn, streaming)  # all or none: no loop mixes the policies
        for r in streaming:
            assert r["loads"] == 8, (kern, fn, r)           # label bytes + new depth + six record planes
            assert r["scratch"] == 0 and r["flat"] == 0 and r["stores"] == 0, (kern, fn, r)
            assert r["waits"][-2:] == [2, 0] and all(w > 0 for w in r["waits"][:-1]), (kern, fn, r)  # one full wait per trip, at its end
