"""The IRLS passes load the records of a sweep with one of two policies per trip (sf_irls.h: pass_division):
the last `window` pixels a sweep walks with the default policy, everything before them non-temporally. A load policy decides where
a line is kept, never what a load returns: the visiting order, the trip counts, pass 1's flush cadence and the order of every sum
are those of the undivided loops. So every result is BIT-identical to the all-default run -- no tolerance anywhere, the fp64
||res||^2 (through res_sqnorm -> est_cov -> the velocity filter -> twist_level, T, twist) included.

Cases and inputs are those of tests/test_gpu_serpentine.py (imported): n0 % 64 = 48 and 16, the label plane, pairs that straddle
columns, a one-level pyramid, a level of fewer pixels than one trip (an empty nt range; lanes that make no trip) and, on the cluster
build, workgroups whose range starts at px_begin > 0. Every case runs with SF_PASS_POLICY=default (the reference of the comparison)
and with SF_PASS_WINDOW_PX = 0 (every record nt), 1 (one trip), 2 * threads + 1 (the division inside the level, off the trip grid)
and 2^30 (the whole level default), in the serpentine order and once more with SF_SOLVER_FORWARD=1 (the window at the top of
pass 2's range instead of at its bottom), on all three builds of the frame kernel (`hip` fixture).
"""
import os

import numpy as np
import pytest

from staticfusion_amd import _capi as capi
from conftest import make_solver
from test_exact_references import TWIST_OLD
from test_gpu_serpentine import CASES, TRACE_SCALARS, TRACE_VECTORS, _pair

pytestmark = pytest.mark.gpu

PLANES = (capi.LIN_DCU, capi.LIN_DCV, capi.LIN_DCT, capi.LIN_DDU, capi.LIN_DDV, capi.LIN_DDT, capi.LIN_WC, capi.LIN_WD, capi.LIN_NULL)


def _solve(api, name, forward, policy=None, window=None):
    rows, cols, mk, _ = CASES[name]
    env = {"SF_SOLVER_FORWARD": "1" if forward else None, "SF_PASS_POLICY": policy,
           "SF_PASS_WINDOW_PX": None if window is None else str(window)}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        s = make_solver(api, rows, cols, mk(api), _pair(name))
        s.set_twist_old(0, TWIST_OLD)
        s.build_pyramid(True)
        s.run_solver(True)
        s.synchronize()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return s


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _snapshot(s):
    st = s.stats()
    out = {"counts": (st.n_irls, st.n_outer, st.status)}
    for i in range(st.n_outer):
        for f in TRACE_SCALARS:
            out["trace%d.%s" % (i, f)] = _bits(getattr(st.outer[i], f)) if f == "aver_res" else getattr(st.outer[i], f)
        for f in TRACE_VECTORS + ("twist_level", "T"):
            out["trace%d.%s" % (i, f)] = _bits(getattr(st.outer[i], f)[:])
    if s.params.segmentation_enabled:
        for L in range(s.levels):
            out["labels%d" % L] = s.labels(L)
    for which in PLANES:
        out["plane%d" % which] = _bits(s.lin_plane(which))
    out["T"] = _bits(s.T())
    out["twist"] = _bits(s.twist())
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_results_do_not_depend_on_the_load_policy(hip, name):
    for forward in (False, True):
        ref_solver = _solve(hip, name, forward, policy="default")
        threads = ref_solver.variant()[1]
        ref = _snapshot(ref_solver)
        assert ref["counts"][0] > ref["counts"][1], "the case never ran a second IRLS iteration: no hand-over between the passes"
        for window in (0, 1, 2 * threads + 1, 1 << 30):
            got = _snapshot(_solve(hip, name, forward, window=window))
            assert got.keys() == ref.keys(), (forward, window)
            for key in ref:
                same = np.array_equal(ref[key], got[key]) if isinstance(ref[key], np.ndarray) else ref[key] == got[key]
                assert same, (name, hip.default_variant, "forward" if forward else "serpentine", "window %d" % window, key)
