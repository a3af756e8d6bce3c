"""The solver of the deformation graphs (sfd_solve, staticfusion_amd/csrc/sf_deform_solve.h), checks that need no GPU. The
library is held to tests/deform_ref.py bit for bit -- every transform and every reported energy -- on: 25 nodes on a plane with
one edge pulled 5 cm and the other pinned; constraints that are one rigid motion of 12 nodes with no pins; one node without
damping (SFD_DEGENERATE) and with; a constraint no node is eligible for (counted, not bound); zero constraints (the identity
stays). Properties are asserted on the restatement's own output.

THE RIGID BAR. Constraints that are one rigid motion x -> R x + t have the exact solution M_j = [R | R g_j + t - g_j] for every
node. tests/deform_ref.py leaves max |M - M_exact| = 5.96e-08 there (measured on the CPU, fp64 solve rounded to float: half
an ulp of the entries near 1); the bar is ten times that, RIGID_BAR = 5.96e-07. The margin covers another fp64 path without a
libm only.

THE ENERGIES NEVER RISE -- beyond what rounding moves them. Gauss-Newton stops changing the transforms at a fixed point, and
from there the energy it reports is the same number up to the rounding of its own evaluation. A residual is a short fp64 chain
over coordinates of magnitude <= s (s = 2 here): its error is at most delta = 16 * 2^-53 * s. With E = sum w |r|^2, moving
every r by delta moves E by at most 2 delta sum w |r| <= 2 delta sqrt(sum w) sqrt(E) (Cauchy-Schwarz). So the assertion is
E[k + 1] <= E[k] + 2 delta sqrt(W) sqrt(E[k]) with W the sum of all weights; that allowance is ~1e-16 where the energies are
~1e-6 and is nothing while the solver still makes progress."""
import numpy as np
import pytest

import deform_cases as dc
import deform_ref as dr

F = np.float32
RIGID_LEFT = 5.96e-08   # what the restatement leaves in the rigid case (measured; asserted below to within 2 %)
RIGID_BAR = 10 * RIGID_LEFT


def cases():
    """(name, pos, times, src, dst, constraint times, weights, solve parameters that differ from the defaults)"""
    pos, times, src, dst = dc.plane_pull()
    rpos, rtimes, rsrc, rdst, _, _ = dc.rigid_case()
    one = np.array([[0.5, 0.5, 0.5]], F)
    late = np.zeros(src.shape[0], F)
    late[3] = 50.0  # no node lies within the window of this one
    none = np.zeros((0, 3), F)
    return [("pull", pos, times, src, dst, np.zeros(src.shape[0], F), np.ones(src.shape[0], F), {}),
            ("rigid", rpos, rtimes, rsrc, rdst, np.zeros(40, F), np.ones(40, F), dict(damping=0.0)),
            ("one_node", one, np.zeros(1, F), [[0.6, 0.5, 0.5]], [[0.6, 0.5, 0.6]], np.zeros(1, F), np.ones(1, F), dict(damping=0.0)),
            ("one_node_damped", one, np.zeros(1, F), [[0.6, 0.5, 0.5]], [[0.6, 0.5, 0.6]], np.zeros(1, F), np.ones(1, F), dict(damping=1e-3)),
            ("unbound", pos, times, src, dst, late, np.full(src.shape[0], 2.0, F), dict(time_window=1.0, iterations=5)),
            ("none", pos, times, none, none, np.zeros(0, F), np.zeros(0, F), {})]


@pytest.fixture(scope="module")
def reference():
    return {c[0]: dr.solve(*c[1:7], **c[7]) for c in cases()}


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_the_library_equals_the_restatement_bit_for_bit(case, reference):
    from staticfusion_amd import deform

    name, pos, times, src, dst, ct, wts, kw = case
    M, rep = deform.solve(pos, times, src, dst, ct, wts, params=deform.SolveParams(**kw))
    want_M, want = reference[name]
    print(name, rep["status"], rep["iterations_done"], rep["n_bound"], rep["energy"])
    assert np.array_equal(M, want_M)
    assert np.array_equal(rep["energy"], want["energy"])
    assert {k: rep[k] for k in ("status", "iterations_done", "n_bound", "n_unbound")} == {k: want[k] for k in ("status", "iterations_done", "n_bound", "n_unbound")}


def test_properties_of_the_restatements_output(reference):
    identity = np.eye(3, 4, dtype=F)
    for name, pos, times, src, dst, ct, wts, kw in cases():
        M, rep = reference[name]
        E = rep["energy"]
        assert E.shape[0] == rep["iterations_done"] + 1 and np.all(E >= 0)
        p = dict(dr.SOLVE_DEFAULTS, **kw)
        W = float(np.sum(wts)) + p["w_reg"] * int((dr.edges(pos, times, p["time_window"]) >= 0).sum())
        delta = 16 * 2.0 ** -53 * 2.0
        allowance = 2 * delta * np.sqrt(W) * np.sqrt(E[:-1])
        print(name, "energy steps", np.diff(E), "allowance", allowance)
        assert np.all(E[1:] <= E[:-1] + allowance), name  # the reported energies never rise
    M, rep = reference["pull"]
    assert rep["status"] == dr.OK and rep["iterations_done"] == 8 and rep["n_bound"] == 10 and rep["n_unbound"] == 0
    assert rep["energy"][-1] < 1e-3 * rep["energy"][0]
    pos = cases()[0][1]
    far, near = pos[:, 0] == pos[:, 0].max(), pos[:, 0] == 0
    assert np.all(np.abs(M[far, 2, 3] - 0.05) < 2e-3) and np.all(np.abs(M[near, :, 3]) < 2e-3)  # pulled 5 cm; pinned
    mid = M[pos[:, 0] == F(0.5), 2, 3]
    assert np.all((mid > 0.01) & (mid < 0.04))  # the correction is spread over the nodes between
    # one node, one constraint: rotation about the line through node and constraint is not observable
    M, rep = reference["one_node"]
    assert rep["status"] == dr.DEGENERATE and rep["iterations_done"] == 0 and rep["energy"].shape == (1,) and np.array_equal(M[0], identity)
    M, rep = reference["one_node_damped"]
    assert rep["status"] == dr.OK and rep["iterations_done"] == 8 and rep["energy"][-1] < 1e-12
    # a constraint no node is eligible for is counted and not bound
    M, rep = reference["unbound"]
    assert (rep["n_bound"], rep["n_unbound"], rep["iterations_done"]) == (9, 1, 5)
    # no constraints: the identity stays, and every energy is 0
    M, rep = reference["none"]
    assert rep["status"] == dr.OK and np.array_equal(M, np.tile(identity, (25, 1, 1))) and not np.any(rep["energy"])


def test_the_rigid_case_returns_the_motion_for_every_node(reference):
    from staticfusion_amd import deform

    pos, times, src, dst, R, t = dc.rigid_case()
    exact = dc.rigid_M(pos, R, t).astype(np.float64)
    M, rep = reference["rigid"]
    left = np.abs(M.astype(np.float64) - exact).max()
    print("the restatement leaves", left, "bar", RIGID_BAR)
    assert rep["status"] == dr.OK and abs(left - RIGID_LEFT) <= 0.02 * RIGID_LEFT  # the figure the bar was taken from still holds
    c = [c for c in cases() if c[0] == "rigid"][0]
    got, _ = deform.solve(*c[1:7], params=deform.SolveParams(**c[7]))
    assert np.abs(got.astype(np.float64) - exact).max() <= RIGID_BAR
