"""rdc_solid_newton_dist across 2 and 3 ranks (tests/solid_newton_dist_ranks.py: spawned rank processes, gloo, every rank on GPU 0)
on the two shipped solid cases, against the numpy Newton of tests/solid_newton_ref.py on the GLOBAL system, which knows no partition:
trajectory, positions with the ghost coordinates bit for bit their owners', the callbacks the entry makes itself, halving, inexact
Newton, the preconditioners and methods of the partitioned linear entries, refusals, an aborting callback, and world size 1 against
rdc_solid_newton.  One spawn per (case, world); the reference runs are those of tests/test_gpu_solid_newton.py, computed once."""
from types import SimpleNamespace

import numpy as np
import pytest

import solid_newton_dist_ranks as R
import solid_newton_ref as N
from rdcfes_amd import AssemblyContext, SolveComm
from rdcfes_amd.context import (ERR_COMM, ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED, NEWTON_CONVERGED_RESIDUAL, NEWTON_CONVERGED_STEP,
                                NEWTON_MAX_ITS)
from test_gpu_solid_newton import CASES, MARGIN, TIGHT, TOL, _ref
from test_solid_newton_ref import HALVING_CAP

pytestmark = pytest.mark.gpu
WORLDS = (2, 3)
ITERATIONS = {("cube", 0.1): 2, ("cube", 1.0): 4, ("hydrogel", 0.1): 2}         # tight: converged by residual
INEXACT_ITERATIONS = {("cube", 0.1): 2, ("cube", 1.0): 4, ("hydrogel", 0.1): 3}  # shipped options: converged by step
assert TIGHT == R.TIGHT
I = {f: k for k, f in enumerate(R.INFO_FIELDS)}


def _same_on_every_rank(runs):
    a = runs[0]
    for b in runs[1:]:
        assert b["info"] == a["info"]
        for k in ("residuals", "steps", "lin_its", "lin_reasons"):
            assert b[k].tobytes() == a[k].tobytes(), k


def _gather(ranks, runs):
    """the global coordinates from the owned rows of the ranks"""
    n = sum(rk["n_owned"] for rk in ranks)
    X = np.full((n, 3), np.nan)
    for rk, r in zip(ranks, runs):
        X[rk["node_global"][:rk["n_owned"]]] = r["xyz"][:rk["n_owned"]]
    assert np.all(np.isfinite(X))
    return X


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name,pt", CASES)
def test_trajectory_against_the_global_reference(oracle, name, pt, world):
    ref = _ref(oracle, name, pt, 1e-10, **TIGHT)
    exact = _ref(oracle, name, pt, "exact", **TIGHT)
    ranks = R.run(name, world)
    runs = [rk[("tight", pt)] for rk in ranks]
    _same_on_every_rank(runs)
    d = runs[0]
    info = d["info"]
    assert info[I["reason"]] == ref["reason"] == NEWTON_CONVERGED_RESIDUAL
    assert info[I["nonlinear_iterations"]] == ref["nonlinear_iterations"] == ITERATIONS[(name, pt)]
    assert info[I["assemblies"]] == info[I["nonlinear_iterations"]] + 1 and info[I["halvings"]] == 0 and np.all(d["steps"] == 1.0)
    assert info[I["linear_iterations"]] == int(d["lin_its"].sum()) and np.all(d["lin_reasons"] == 0)
    got = list(d["residuals"]) + [info[I["last_residual"]]]
    assert len(got) == len(ref["residuals"]) == len(exact["residuals"])
    worst = 0.0
    for i, (g, r, e) in enumerate(zip(got, ref["residuals"], exact["residuals"])):
        floor = abs(r - e)       # the reference's own deviation between its bicgstab(1e-10) and spsolve runs
        if floor > 0:
            worst = max(worst, abs(g - r) / floor)
        print(f"{name} {pt} world {world} it {i}: device {g:.10e} ref {r:.10e} exact {e:.10e} | dev-ref {abs(g - r):.2e} floor {floor:.2e} "
              f"| 1e-10 first {TOL * ref['first_residual']:.2e} | linear its {d['lin_its'][i] if i < len(d['lin_its']) else '-'}")
        assert abs(g - r) <= MARGIN * floor + TOL * ref["first_residual"], (i, g, r, floor)
    print(f"{name} {pt} world {world}: worst ratio to the floor {worst:.2f}")


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name,pt", CASES)
def test_positions_and_ghost_coordinates(oracle, name, pt, world):
    ref = _ref(oracle, name, pt, 1e-10, **TIGHT)
    exact = _ref(oracle, name, pt, "exact", **TIGHT)
    ranks = R.run(name, world)
    runs = [rk[("tight", pt)] for rk in ranks]
    X = _gather(ranks, runs)
    floor = float(np.abs(ref["xyz"] - exact["xyz"]).max())
    bound = MARGIN * floor + TOL * float(np.abs(ref["xyz"]).max())
    dev = float(np.abs(X - ref["xyz"]).max())
    print(f"{name} {pt} world {world}: max |x_device - x_ref| {dev:.3e}, floor {floor:.3e}, bound {bound:.3e}")
    assert dev <= bound
    # every ghost coordinate is its owner's, bit for bit -- from a start in which every ghost coordinate was wrong
    n_ghost = 0
    for me, (rk, r) in enumerate(zip(ranks, runs)):
        for q, ids in rk["ghosts_of"].items():
            src = ranks[q]["sends_to"][me]
            assert r["xyz"][ids].tobytes() == runs[q]["xyz"][src].tobytes(), (me, q)
            n_ghost += len(ids)
    assert n_ghost == sum(rk["n_nodes"] - rk["n_owned"] for rk in ranks) > 0
    # each context holds the oracle's residual at the returned coordinates on its owned rows
    _, Rg = N.assemble(oracle, N.at(N.system(name), pt), X, jacobian=False)
    first = runs[0]["info"][I["first_residual"]]
    for k, (rk, r) in enumerate(zip(ranks, runs)):
        want = Rg.reshape(-1, 3)[rk["node_global"][:rk["n_owned"]]].reshape(-1)
        err = float(np.linalg.norm(r["rhs"] - want))
        print(f"{name} {pt} world {world} rank {k}: |rhs - oracle| {err:.3e}, 1e-10 max(|R|, first) {TOL * max(np.linalg.norm(Rg), first):.3e}")
        assert r["rhs"].size == want.size and err <= TOL * max(float(np.linalg.norm(Rg)), first)


def _own_callbacks(d):
    """(exchanges into the coordinate ghost tail, all-reduces of 8 doubles) of a logged run"""
    log = d["log"]
    to_tail = [k for k, e in enumerate(log) if e[0] == "exchange" and e[1] == d["tail"]]
    return to_tail, sum(1 for e in log if e == ("allreduce", 8))


@pytest.mark.parametrize("method", ["bicgstab", "gmres"])
def test_the_callbacks_of_the_loop_itself(method):
    ranks = R.run("cube", 2)
    runs = [rk[("callbacks", method)] for rk in ranks]
    _same_on_every_rank(runs)
    for d in runs:
        to_tail, n8 = _own_callbacks(d)
        assert to_tail == [0], to_tail                                   # exactly one, and it is the first callback
        assert d["first_send"].shape == d["want_send"].shape and d["first_send"].tobytes() == d["want_send"].tobytes()
        its = d["info"][I["nonlinear_iterations"]]
        assert d["info"][I["reason"]] == NEWTON_CONVERGED_RESIDUAL and its == ITERATIONS[("cube", 0.1)]
        assert n8 == 2 * its + 1, (n8, its)
        kinds = {e[0] for e in d["log"]}
        assert ("wide" in kinds) == (method == "gmres") and "sized" not in kinds
        assert max(e[1] for e in d["log"] if e[0] == "allreduce") == 8 and sum(1 for e in d["log"] if e[0] == "exchange") > 1


def test_halving(oracle):
    kw = dict(TIGHT, require_reduction=True, max_nonlinear_iterations=HALVING_CAP)
    ref = _ref(oracle, "cube", 1.5, 1e-10, **kw)
    assert min(ref["gaps"]) >= 2e-2 and ref["halvings"] >= 1     # a property of the reference, whatever the partition
    ranks = R.run("cube", 2)
    runs = [rk["halving"] for rk in ranks]
    _same_on_every_rank(runs)
    for d in runs:
        info = d["info"]
        print(f"halving: steps {list(d['steps'])}, halvings {info[I['halvings']]}, assemblies {info[I['assemblies']]}, residuals {list(d['residuals'])}")
        assert list(d["steps"]) == ref["steps"] == [1.0, 0.25, 0.125]
        assert info[I["halvings"]] == ref["halvings"] == 5 and info[I["assemblies"]] == ref["assemblies"] == 12
        assert info[I["reason"]] == ref["reason"] == NEWTON_MAX_ITS
        assert np.all(np.isfinite(d["residuals"])) and np.isfinite(info[I["last_residual"]])
        to_tail, n8 = _own_callbacks(d)
        its, closing = info[I["nonlinear_iterations"]], 0                # no stop by step: no measuring accept
        full = its + 1                                                   # one per iteration and the one that found the cap
        assert to_tail == [0] and n8 == full + its + info[I["halvings"]] + closing == 12


@pytest.mark.parametrize("name,pt", CASES)
def test_inexact_newton_with_the_shipped_options(oracle, name, pt):
    opt = N.shipped_options(name)
    lin = dict(rel_tol=opt.pop("rel_tol"), max_its=opt.pop("max_its"))
    s = N.at(N.system(name), pt)
    ref = N.newton(oracle, s, s.xyz, N.bicgstab_linear(lin["rel_tol"], max_its=lin["max_its"]), **opt)
    runs = [rk[("inexact", pt)] for rk in R.run(name, 2)]
    _same_on_every_rank(runs)
    d = runs[0]
    print(f"{name} {pt}: linear iterations {list(d['lin_its'])} (reference {ref['lin_its']}), residuals {list(d['residuals'])}")
    assert d["info"][I["reason"]] == ref["reason"] == NEWTON_CONVERGED_STEP
    assert d["info"][I["nonlinear_iterations"]] == ref["nonlinear_iterations"] == INEXACT_ITERATIONS[(name, pt)]


@pytest.mark.parametrize("what", sorted(R.THROUGH))
def test_preconditioners_and_methods_pass_through(oracle, what):
    ref = _ref(oracle, "cube", 0.1, 1e-10, **TIGHT)
    runs = [rk[("through", what)] for rk in R.run("cube", 2)]
    _same_on_every_rank(runs)
    d = runs[0]
    info = d["info"]
    print(f"{what}: linear iterations {list(d['lin_its'])}, residuals {list(d['residuals'])} last {info[I['last_residual']]:.3e}")
    assert info[I["reason"]] == NEWTON_CONVERGED_RESIDUAL and info[I["nonlinear_iterations"]] == ref["nonlinear_iterations"] == 2
    assert info[I["linear_iterations"]] == int(d["lin_its"].sum()) and np.all(d["lin_reasons"] == 0)
    assert info[I["last_residual"]] <= max(1e-8, 1e-8 * info[I["first_residual"]])


def test_refusals():
    for rk in R.run("cube", 2):
        ref = rk["refusals"]
        p4 = ref["precond4"]                     # the linear entry's own refusal: back from the first solve, nothing has moved
        assert p4["code"] == ERR_UNSUPPORTED and p4["owned_unchanged"]
        for k in ("mg_without_sized", "gmres_without_wide"):
            assert ref[k]["code"] == ERR_INVALID and ref[k]["log"] == [] and ref[k]["owned_unchanged"], k
        assert ref["no_plan"]["code"] == ERR_STATE and ref["no_plan"]["log"] == [] and ref["no_plan"]["owned_unchanged"]
        bad = [k for k in ref if isinstance(k, tuple)]
        assert len(bad) == 6
        for k in bad:
            assert ref[k]["code"] == ERR_INVALID and ref[k]["log"] == [] and ref[k]["owned_unchanged"], k


def test_a_callback_that_aborts(oracle):
    ranks = R.run("cube", 2)
    for rk in ranks:
        ab = rk["abort"]
        assert ab["code"] == ERR_COMM
        assert ab["last"] == ("allreduce", 8) and ab["n8"] == 2          # the failing call is the last callback made
        assert ab["finite"] and ab["moved"]                              # the step before it had been taken
    # the same contexts, coordinates uploaded again: the result of the tight run
    after, tight = [rk["after_abort"] for rk in ranks], [rk[("tight", 0.1)] for rk in ranks]
    _same_on_every_rank(after)
    assert after[0]["info"][I["reason"]] == NEWTON_CONVERGED_RESIDUAL
    assert after[0]["info"][I["nonlinear_iterations"]] == tight[0]["info"][I["nonlinear_iterations"]] == 2
    first = tight[0]["info"][I["first_residual"]]
    assert abs(after[0]["info"][I["first_residual"]] - first) <= TOL * first
    # positions: the bound of the tight run against the reference
    ref, exact = _ref(oracle, "cube", 0.1, 1e-10, **TIGHT), _ref(oracle, "cube", 0.1, "exact", **TIGHT)
    bound = MARGIN * float(np.abs(ref["xyz"] - exact["xyz"]).max()) + TOL * float(np.abs(ref["xyz"]).max())
    assert float(np.abs(_gather(ranks, after) - ref["xyz"]).max()) <= bound


def test_world_size_one_is_the_plain_entry():
    """ghost-free context, a communicator of world size 1, the deterministic assembly ("solid_kernel" = 2)"""
    s = N.at(N.system("cube"), 0.1)
    lp = SimpleNamespace(rank=0, send_ids={}, recv_ids={}, xyz=s.xyz, n_owned=s.xyz.shape[0])
    kw = dict(TIGHT, rel_tol=1e-10, max_its=50000)
    with AssemblyContext(0) as ctx:
        ctx.set_option("solid_kernel", 2)
        s.upload(ctx)
        comm = SolveComm(lp, 3, "cuda:0", wide=True)

        def call(dist):
            ctx.mesh_update_coords(s.xyz)
            info = ctx.solid_newton_dist(comm, s.params, **kw) if dist else ctx.solid_newton(s.params, **kw)
            hist = ctx.solid_newton_history()
            return R.info_tuple(info), tuple(h.tobytes() for h in hist), ctx.coords_tensor().cpu().numpy().copy()

        a, b, d = call(False), call(False), call(True)
        assert comm.exchanges >= 1 and comm.allreduces >= 2 * a[0][I["nonlinear_iterations"]] + 1
    assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes(), "two rdc_solid_newton calls differ under solid_kernel = 2"
    assert d[0] == a[0] and d[1] == a[1]
    assert d[2].tobytes() == a[2].tobytes()
