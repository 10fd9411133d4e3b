"""Pins the numpy Newton of tests/solid_newton_ref.py (the yardstick of rdc_solid_newton) on the two shipped solid cases, from the
undeformed mesh: the trajectories with an exact linear solve, the stop by step, the halving case and the condition under which
the device may be required to take the same accept / reject branches."""
import numpy as np
import pytest

import solid_newton_ref as N

NO_STEP_STOP = dict(max_nonlinear_iterations=10, require_reduction=False, relative_step_tolerance=0.0,
                    relative_residual_tolerance=1e-8, absolute_residual_tolerance=1e-8)
# ||R|| of every full assembly with an exact linear solve, to 2 digits
TABLE = {("cube", 0.1): [1.978e6, 5.2e-1, 8.9e-3],
         ("cube", 1.0): [1.978e7, 1.0e2, 3.8e1, 4.5, 1.4e-1],
         ("hydrogel", 0.1): [3.49e-4, 3.9e-7, 9.5e-9],
         ("hydrogel", 1.0): [3.49e-3, 3.1e-5, 5.6e-6, 6.3e-7, 9.3e-8, 1.5e-8, 2.5e-9]}
# linear iterations with solve_ref.bicgstab(precond=2, rel_tol=1e-3)
INEXACT = {("cube", 0.1): [12, 13], ("cube", 1.0): [12, 21, 19, 20],
           ("hydrogel", 0.1): [36, 63, 58], ("hydrogel", 1.0): [36, 60, 61, 46, 40, 36]}
HALVING_CAP = 3   # iterations of the halving case the GPU test follows: every comparison inside them has a gap >= 1e-6 (below)


def _run(oracle, name, pt, linear, **kw):
    s = N.at(N.system(name), pt)
    return N.newton(oracle, s, s.xyz, linear, **kw)


@pytest.mark.parametrize("name,pt", sorted(TABLE))
def test_trajectory_with_an_exact_linear_solve(oracle, name, pt):
    r = _run(oracle, name, pt, N.spsolve_linear, **NO_STEP_STOP)
    want = TABLE[(name, pt)]
    assert r["reason"] == N.CONVERGED_RESIDUAL and r["nonlinear_iterations"] == len(want) - 1 == len(r["steps"])
    assert r["assemblies"] == len(want) and r["halvings"] == 0 and all(st == 1.0 for st in r["steps"])
    assert len(r["residuals"]) == len(want)
    for got, w in zip(r["residuals"], want):
        assert abs(got - w) <= 0.05 * w, (got, w)       # 2 digits: half a unit of the second digit is at most 5 %
    assert r["first_residual"] == r["residuals"][0] and r["last_residual"] == r["residuals"][-1]
    assert r["last_residual"] <= max(1e-8, 1e-8 * r["first_residual"])


@pytest.mark.parametrize("name,pt", sorted(INEXACT))
def test_inexact_newton_has_the_linear_counts_of_the_issue(oracle, name, pt):
    r = _run(oracle, name, pt, N.bicgstab_linear(1e-3), **NO_STEP_STOP)
    assert r["reason"] == N.CONVERGED_RESIDUAL and r["lin_its"] == INEXACT[(name, pt)]
    assert r["linear_iterations"] == sum(r["lin_its"]) and r["nonlinear_iterations"] == len(r["lin_its"])


def test_the_cube_stops_by_step_after_two_iterations(oracle):
    r = _run(oracle, "cube", 0.1, N.spsolve_linear, **dict(NO_STEP_STOP, relative_step_tolerance=1e-3))
    assert r["reason"] == N.CONVERGED_STEP and r["nonlinear_iterations"] == 2
    assert r["assemblies"] == 3 and len(r["residuals"]) == 2            # two full assemblies and the closing residual-only one
    assert r["last_step_norm"] <= 1e-3 * r["last_solution_norm"]
    assert abs(r["last_residual"] - 8.9e-3) <= 0.05 * 8.9e-3


def test_max_iterations(oracle):
    r = _run(oracle, "cube", 1.0, N.spsolve_linear, **dict(NO_STEP_STOP, max_nonlinear_iterations=2))
    assert r["reason"] == N.MAX_ITS and r["nonlinear_iterations"] == 2 and r["assemblies"] == 3


def test_halving_case(oracle):
    """cube at pseudo_time 1.5 under require_reduction: iteration 1 takes the full step, iteration 2 two halvings, iteration 3 three"""
    r = _run(oracle, "cube", 1.5, N.spsolve_linear, **dict(NO_STEP_STOP, require_reduction=True, max_nonlinear_iterations=HALVING_CAP))
    assert r["reason"] == N.MAX_ITS and r["steps"] == [1.0, 0.25, 0.125] and r["halvings"] == 5
    assert r["assemblies"] == (HALVING_CAP + 1) + (1 + 3 + 4)           # full assemblies + trials
    assert np.all(np.isfinite(r["residuals"])) and all(np.isfinite(t[2]) for t in r["trials"])
    for got, w in zip(r["residuals"], [2.97e7, 5.16e2, 3.98e2, 3.89e2]):
        assert abs(got - w) <= 0.005 * w
    # the condition under which the device may be held to the same branches: no comparison is closer than 1e-6
    assert len(r["gaps"]) == len(r["trials"]) == 8 and min(r["gaps"]) >= 1e-6, r["gaps"]


def test_a_nan_start_is_not_finite_and_stays(oracle):
    s = N.at(N.system("cube"), 0.1)
    x0 = s.xyz.copy()
    x0[5, 1] = np.nan
    r = N.newton(oracle, s, x0, N.spsolve_linear, **NO_STEP_STOP)
    assert r["reason"] == N.NOT_FINITE and r["nonlinear_iterations"] == 0 and r["assemblies"] == 1
    assert np.array_equal(r["xyz"], x0, equal_nan=True)
