"""IRLS pass 2 walks its records back down from where pass 1 ended (sf_irls.h: irls_pass2<VAR, DIR = 1>);
SF_SOLVER_FORWARD=1 selects the old upward walk per launch. Every case solves the same inputs on a forward handle and on a
serpentine handle of the same build of the frame kernel (`hip` fixture: throughput, latency, cluster).

Bit-identical between the two: n_irls, n_outer, every trace entry's level / k / n_valid / irls_iters / aver_res / b_segm / var /
AtA / AtB, the labels of every level and the record planes of the last outer iteration. The per-label sums of pass 2 are
Q32.32 integers and pass 1 is untouched, so nothing that steers the iteration can move.

Allowed to move by the order of ONE fp64 sum (||res||^2 -> res_sqnorm -> est_cov -> the velocity filter): twist_level, T, twist.
est_cov itself is not readable through the ABI; the filter is its only consumer. Their bound is measured, not fixed in advance:
the distance of each order to the fp64 reference of tests/exact_ref.py (filter_reference of test_exact_references.py, from the
handle's own rows, solution and AtA -- identical in both orders, so the reference is computed once), and the serpentine order
may be at most as far as the forward order plus the forward order's own spread between the 4- and the 5-per-CU compilation of
the throughput build on the same case.

Figures of one run (one MI355X, the six cases on all three builds):
  forward order's spread between its 4- and 5-per-CU kernels: 0 in every quantity of every case (bit-identical);
  |serpentine - forward|: 0 in twist_level, T and twist of every case on every build (the fp64 sums differ below the float
  rounding of res_sqnorm), so both orders are at the same distance from the reference: max |twist_level - exact| 2.1e-11 ..
  1.6e-9, |T - exact| 2.5e-8 .. 4.7e-8, |twist - exact| 1.0e-10 .. 6.0e-9, max |twist_level - exact| / bound 5.6e-5 .. 0.0085.
"""
import os

import numpy as np
import pytest

import exact_ref as E
from conftest import driver_params, make_solver
from staticfusion_amd import _capi as capi
from staticfusion_amd.synth import make_pair
from test_exact_references import TWIST_OLD, _partial_wave, _tiny, filter_reference, irls_inputs

pytestmark = pytest.mark.gpu


def _odo(a, levels):  # pure odometry WITH the velocity filter: res_sqnorm reaches the pose
    return driver_params(a, kb=1.5, ctf_levels=levels, segmentation_enabled=0, debug_planes=1)


def _seg(a, levels):
    return driver_params(a, kb=1.5, ctf_levels=levels, debug_planes=1)


# name -> (rows, cols, params(api), pair factory)
CASES = {
    "20x44": (20, 44, lambda a: _odo(a, 2), lambda: _partial_wave(20, 44)),                                 # n0 % 64 = 48
    "40x42_seg": (40, 42, lambda a: _seg(a, 3), lambda: _partial_wave(40, 42)),                             # n0 % 64 = 16, segmentation on
    "odd_45x48": (45, 48, lambda a: _odo(a, 2), lambda: make_pair(seed=6, sphere=False, out_rows=45, out_cols=48)),    # pairs straddle columns
    "odd_36x117": (36, 117, lambda a: _odo(a, 1), lambda: make_pair(seed=9, sphere=True, out_rows=36, out_cols=117)),  # n0 % 64 = 52; one level: 18 x 58 is no multiple of 4
    "single_trip_32x48": (32, 48, lambda a: _seg(a, 2), _tiny),                                             # level 1: 384 pixels < 2 x 256
    "shared_120x160_seg": (120, 160, lambda a: _seg(a, 3), lambda: make_pair(seed=11, sphere=True, out_rows=120, out_cols=160)),  # cluster: px_begin > 0
}
_pairs, _spread = {}, {}


def _pair(name):
    if name not in _pairs:
        _pairs[name] = CASES[name][3]()
    return _pairs[name]


def _solve(api, name, forward, wg_per_cu=None):
    rows, cols, mk, _ = CASES[name]
    env = {"SF_SOLVER_FORWARD": "1" if forward else None, "SF_THROUGHPUT_WG_PER_CU": wg_per_cu}
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


def _moving(s):
    """the results the order of the fp64 sum may move: (twist_level of the last outer iteration, T, twist)"""
    st = s.stats()
    return (np.array(st.outer[st.n_outer - 1].twist_level, np.float64), s.T().astype(np.float64), s.twist().astype(np.float64))


def _forward_spread(name):
    """max |4-per-CU - 5-per-CU| of the forward order on the throughput build, per quantity (once per case)"""
    if name not in _spread:
        import staticfusion_amd as sf

        thr = sf.load().with_variant("throughput")
        m4, m5 = (_moving(_solve(thr, name, True, n)) for n in ("4", "5"))
        _spread[name] = [float(np.abs(x - y).max()) for x, y in zip(m4, m5)]
    return _spread[name]


TRACE_SCALARS = ("level", "k", "n_valid", "irls_iters", "aver_res")
TRACE_VECTORS = ("b_segm", "b_prior", "lambda_t_w", "var", "AtA", "AtB")


@pytest.mark.parametrize("name", sorted(CASES))
def test_serpentine_order_against_forward_order(hip, name):
    fw, sp = _solve(hip, name, True), _solve(hip, name, False)
    a, b = fw.stats(), sp.stats()
    assert (a.n_irls, a.n_outer, a.status) == (b.n_irls, b.n_outer, b.status)
    assert a.n_irls > a.n_outer, "the case never ran a second IRLS iteration: no hand-over between the passes"
    for i in range(a.n_outer):
        for f in TRACE_SCALARS:
            assert getattr(a.outer[i], f) == getattr(b.outer[i], f), (i, f, getattr(a.outer[i], f), getattr(b.outer[i], f))
        for f in TRACE_VECTORS:
            x, y = np.array(getattr(a.outer[i], f)[:], np.float32), np.array(getattr(b.outer[i], f)[:], np.float32)
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (i, f)
    if fw.params.segmentation_enabled:
        for L in range(fw.levels):
            assert np.array_equal(fw.labels(L), sp.labels(L)), L
    for which in (capi.LIN_DCU, capi.LIN_DCV, capi.LIN_DCT, capi.LIN_DDU, capi.LIN_DDV, capi.LIN_DDT, capi.LIN_WC, capi.LIN_WD, capi.LIN_NULL):
        assert np.array_equal(fw.lin_plane(which).view(np.uint32), sp.lin_plane(which).view(np.uint32)), which

    # the fp64 reference of the last outer iteration, from rows / solution / AtA that are the same bits in both orders
    inp = irls_inputs(fw)
    tl, tol = filter_reference(fw, inp)
    T_ref = E.se3_exp(tl) @ inp["T_prev"]
    ref = (tl, T_ref, E.se3_log(T_ref))
    spread = _forward_spread(name)
    mf, ms = _moving(fw), _moving(sp)
    dist_f = [float(np.abs(x - r).max()) for x, r in zip(mf, ref)]
    dist_s = [float(np.abs(x - r).max()) for x, r in zip(ms, ref)]
    moved = [float(np.abs(x - y).max()) for x, y in zip(mf, ms)]
    print("%s %s: n_irls %d n_outer %d; (twist_level, T, twist) distance to the fp64 reference: forward %s serpentine %s; "
          "|serpentine - forward| %s; forward 4- vs 5-per-CU spread %s; max |twist_level - exact| / bound forward %.3g serpentine %.3g"
          % (name, hip.default_variant, a.n_irls, a.n_outer, ["%.3e" % x for x in dist_f], ["%.3e" % x for x in dist_s],
             ["%.3e" % x for x in moved], ["%.3e" % x for x in spread], float((np.abs(mf[0] - tl) / tol).max()),
             float((np.abs(ms[0] - tl) / tol).max())))
    for q, (ds, df, spr) in enumerate(zip(dist_s, dist_f, spread)):
        assert ds <= df + spr, (("twist_level", "T", "twist")[q], ds, df, spr)
