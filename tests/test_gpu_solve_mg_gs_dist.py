"""Multigrid across ranks with the rank-local multicolour Gauss-Seidel smoother (RDC_PRECOND_MULTIGRID_GS_LOCAL, precond 6) through
rdc_solve_dist_mg, rdc_solve_dist_gmres, rdc_solve_dist_gmres_arnoldi and, without ghosts, rdc_solve / rdc_solve_mixed.

World 1 in this process: bitwise what rdc_solve(precond = 3) returns under "mg_smoother" = 1, with the callbacks of precond 3.
Worlds 2 and 3 through tests/solve_dist_mg_gs_ranks.py (gloo ranks sharing GPU 0: correctness only) against the oracle's global
assembly and the numpy yardstick tests/solve_ref_mg_gs_dist.py, whose colours tests/test_host_solve_mg_gs_dist.py shows to be those of
the compiled host code.  "mg_gs_fuse" = 0 is the only way to the per-colour launches (k_gs, k_gs_pack) and to the part of colour 0
that runs inside the level-0 exchange on these sizes (every level of every rank has at most 512 nodes), so everything runs under
both values and must return the same bytes.

ONE cycle against the extended-precision reference (gmres_arnoldi_dist, one step: the first column is D^-1 A M v0 / ||v0||), bound
ld.bound(ld.MARGIN, noise) and ld.MARGIN_MIXED for the mixed form, noise = what numpy's FP64 evaluation of the same operator differs
from the extended-precision one by (mixed: also noise32), as tests/test_gpu_mg_cycle.py builds it.  error / max(noise, 16 eps)
measured on an MI355X is recorded in DESIGN.md 7.2."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import solve_dist_mg_gs_ranks as R
import solve_dist_ranks
import solve_ref
import solve_ref_dist
import solve_ref_mg_gs_dist as Y
import solve_ref_mg_ld as ld
import solve_ref_mixed
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import RdcError, SolveComm, SolveInfo, SolveParams, partition
from rdcfes_amd.context import (ERR_STATE, ERR_UNSUPPORTED, PRECOND_MULTIGRID, PRECOND_MULTIGRID_GS_LOCAL, SOLVE_BAD_DIAGONAL, SOLVE_CONVERGED,
                                SOLVE_MAX_ITS)

pytestmark = pytest.mark.gpu
ASSEMBLY_REL = 1e-10
I = {f: i for i, f in enumerate(solve_dist_ranks.INFO_FIELDS)}
GS, MG = PRECOND_MULTIGRID_GS_LOCAL, PRECOND_MULTIGRID
LD, EPS = ld.LD, ld.EPS


def _world1_comm(s):
    lp = partition.build_local(s.conn, s.xyz, np.zeros(s.conn.shape[0], dtype=np.int32), 0, 1)
    assert lp.n_owned == s.xyz.shape[0] and not lp.send_ids and not lp.recv_ids
    return SolveComm(lp, s.nv, "cuda:0", sized=True, wide=True)


def _counts(c):
    return (c.exchanges, c.sized_exchanges, c.allreduces, c.wide_allreduces)


# ---- 1. the value is known (fails on the parent: "unknown preconditioner 6") ----
def test_precond_6_is_accepted_across_ranks():
    assert GS == 6
    ctx, s, A, rhs, val = _open("hcc_hex")
    with ctx:
        comm = _world1_comm(s)
        xd = _dev(np.zeros(rhs.size))
        a = ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-8, max_its=2000, precond=GS, rhs_scale=s.rhs_scale)
        b = ctx.solve_dist_gmres(comm, xd.data_ptr(), rel_tol=1e-8, max_its=2000, precond=GS, rhs_scale=s.rhs_scale)
        assert a.reason == SOLVE_CONVERGED and b.reason == SOLVE_CONVERGED and a.iterations > 0
    ranks = R.run("hcc_hex", 2)
    assert all(rk[(m, 1e-8, 1)]["info"][I["reason"]] == SOLVE_CONVERGED for rk in ranks for m in ("bicgstab", "gmres"))


# ---- 2. world 1 equals rdc_solve(precond = 3) under "mg_smoother" = 1, bitwise, with the callbacks of precond 3 ----
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex"])
def test_world1_equals_solve_bitwise(name, mixed):
    """pihna_kuhn: level 0 (729 nodes) is above the fused size, so "mg_gs_fuse" = 1 sweeps it colour by colour; hcc_hex: below"""
    ctx, s, A, rhs, val = _open(name)
    tup = solve_dist_ranks.info_tuple
    with ctx:
        comm = _world1_comm(s)
        for method in (0, 1):
            ctx.set_option("solve_method", method)
            dist = ctx.solve_dist_gmres if method else ctx.solve_dist
            for rel_tol in (1e-8, 1e-10):
                kw = dict(rel_tol=rel_tol, max_its=5000, rhs_scale=s.rhs_scale, mixed=mixed)
                x = {k: _dev(np.zeros(rhs.size)) for k in ("ref0", "ref", "six0", "six1", "dist", "dist_f0", "mg", "after0", "after1")}
                ref0 = ctx.solve(x["ref0"].data_ptr(), precond=MG, **kw)                  # smoother 0, before
                ctx.set_option("mg_smoother", 1)
                ref = ctx.solve(x["ref"].data_ptr(), precond=MG, **kw)
                levels, colours = ctx.mg_levels(), ctx.mg_colours()
                six1 = ctx.solve(x["six1"].data_ptr(), precond=GS, **kw)
                ctx.set_option("mg_smoother", 0)
                six0 = ctx.solve(x["six0"].data_ptr(), precond=GS, **kw)
                c0 = _counts(comm)
                got = dist(comm, x["dist"].data_ptr(), precond=GS, **kw)
                c1 = _counts(comm)
                assert ctx.mg_levels() == levels and ctx.mg_colours() == colours
                ctx.set_option("mg_gs_fuse", 0)
                got_f0 = dist(comm, x["dist_f0"].data_ptr(), precond=GS, **kw)
                ctx.set_option("mg_gs_fuse", 1)
                c2 = _counts(comm)
                jac = dist(comm, x["mg"].data_ptr(), precond=MG, **kw)                     # precond 3 on the same communicator
                c3 = _counts(comm)
                after0 = ctx.solve(x["after0"].data_ptr(), precond=MG, **kw)              # a plain solve afterwards is what it was
                ctx.set_option("mg_smoother", 1)
                after1 = ctx.solve(x["after1"].data_ptr(), precond=MG, **kw)
                assert ctx.mg_levels() == levels and ctx.mg_colours() == colours
                ctx.set_option("mg_smoother", 0)
                calls, calls_f0, calls_jac = (tuple(b - a for a, b in zip(p, q)) for p, q in ((c0, c1), (c1, c2), (c2, c3)))
                print(f"{name} mixed {mixed} method {method} tol {rel_tol:g}: {ref.iterations} iterations (smoother 0: {ref0.iterations}), restarts "
                      f"{ref.restarts}, matrix bits {got.matrix_bits}, levels {levels}, colours {colours}; callbacks (exchanges, sized, all-reduces, "
                      f"wide) with 6: {calls}, with 3: {calls_jac} at {jac.iterations} iterations")
                for k, info in (("six0", six0), ("six1", six1), ("dist", got), ("dist_f0", got_f0), ("after1", after1)):
                    assert tup(info) == tup(ref), (k, dict(zip(solve_dist_ranks.INFO_FIELDS, zip(tup(info), tup(ref)))))
                    assert x[k].cpu().numpy().tobytes() == x["ref"].cpu().numpy().tobytes(), f"{k} differs from solve(precond = 3) under mg_smoother = 1"
                assert tup(after0) == tup(ref0) and x["after0"].cpu().numpy().tobytes() == x["ref0"].cpu().numpy().tobytes()
                assert got.reason == SOLVE_CONVERGED and got.matrix_bits == (32 if mixed else 64) and len(levels) >= 3
                assert ref.iterations <= ref0.iterations
                # the callbacks are those of precond 3 on the same communicator at the same iteration count: per iteration and per
                # restart they are linear in the counts, so they are compared through the formulas of the precond-3 tests
                L = len(levels)
                # (the plain solves before it dropped the partitioned hierarchy: the first of the three builds it again, as precond 3
                # does, with one sized exchange and one all-reduce per coarsening step and the all-reduce of the step that stops)
                for info, cc, built in ((got, calls, 1), (got_f0, calls_f0, 0), (jac, calls_jac, 0)):
                    its, restarts = info.iterations, info.restarts
                    if method == 0:
                        nres = 2 + restarts
                        assert cc == (6 * its + nres, 2 * (2 * (L - 2) + 7) * its + built * (L - 1), 3 * its + nres + built * L, 0)
                    else:
                        assert cc == (3 * its + 2 * (restarts + 1) + restarts + 2, (2 * (L - 2) + 7) * (its + restarts + 1) + built * (L - 1),
                                      restarts + 2 + built * L, 2 * its)
        ctx.set_option("solve_method", 0)
        _unchanged(ctx, val, rhs)


# ---- 3. two and three ranks against the global system and the yardstick ----
def _gather(ranks, entry, nv, n_node):
    x = np.full((n_node, nv), np.nan)
    for rk in ranks:
        x[rk["node_global"][:rk["n_owned"]]] = entry(rk)["x"].reshape(-1, nv)[:rk["n_owned"]]
    assert np.all(np.isfinite(x))
    return x


def _ghosts_hold_owner_values(ranks, entry, xg, nv):
    for r, rk in enumerate(ranks):
        loc = entry(rk)["x"].reshape(-1, nv)
        assert loc[rk["n_owned"]:].tobytes() == xg[rk["node_global"][rk["n_owned"]:]].tobytes(), f"ghost rows of rank {r}"


def _same_info(ranks, entry):
    infos = [entry(rk)["info"] for rk in ranks]
    assert all(i == infos[0] for i in infos), infos     # floats compared exactly: identical bits on every rank
    return infos[0]


@pytest.mark.parametrize("method", ["bicgstab", "gmres"])
@pytest.mark.parametrize("name,world", sorted(R.SOLVES_ON))
def test_ranks_against_global_system(oracle, name, world, method):
    s, A, b = solve_ref_dist.global_system(name, oracle)
    ranks = R.run(name, world)
    _, H = Y.hierarchy(name, world, oracle)
    L = H.n_levels
    for rel_tol in R.TOLS:
        e = lambda rk: rk[(method, rel_tol, 1)]
        info, jac = _same_info(ranks, e), _same_info(ranks, lambda rk: rk[(method, rel_tol, "jacobi")])
        xg = _gather(ranks, e, s.nv, s.xyz.shape[0])
        _ghosts_hold_owner_values(ranks, e, xg, s.nv)
        ref = (Y.bicgstab if method == "bicgstab" else Y.gmres)(name, world, oracle, rel_tol)[1]
        f = solve_ref.check_solution(A, b, xg.reshape(-1), s.nv, 2, rel_tol, extra_rel=ASSEMBLY_REL)
        its, restarts = info[I["iterations"]], info[I["restarts"]]
        print(f"{name} world {world} {method} tol {rel_tol:g}: iterations {its} (restarts {restarts}), yardstick {ref['iterations']}, precond 3 on the "
              f"same rig {jac[I['iterations']]}; residual {f['residual_norm']:.3e} <= {f['bound']:.3e}; colours per rank {[e(rk)['colours'] for rk in ranks]}; "
              f"callbacks (exchanges, sized, all-reduces, wide) first solve {[e(rk)['calls_first'] for rk in ranks]}, second {[e(rk)['calls'] for rk in ranks]}")
        assert info[I["reason"]] == SOLVE_CONVERGED and info[I["matrix_bits"]] == 64 and jac[I["reason"]] == SOLVE_CONVERGED
        assert abs(its - ref["iterations"]) <= 2
        assert its <= jac[I["iterations"]]
        assert abs(info[I["rhs_norm"]] - f["rhs_norm"]) <= (1e-13 + ASSEMBLY_REL) * f["rhs_norm"]
        assert abs(info[I["residual_norm"]] - f["residual_norm"]) <= f["rho"]
        assert all(e(rk)["repeat_same"] and rk[(method, rel_tol, 0)]["repeat_same"] for rk in ranks), "a second solve returned other bytes"
        for r, rk in enumerate(ranks):
            f0 = rk[(method, rel_tol, 0)]
            assert f0["x"].tobytes() == e(rk)["x"].tobytes() and f0["info"] == e(rk)["info"], f"rank {r}: mg_gs_fuse 0 and 1 differ"
            assert rk[(method, rel_tol, "smoother1_same")], f"rank {r}: mg_smoother changed the bytes under precond 6"
            assert e(rk)["levels"] == H.level_sizes(r) and e(rk)["colours"] == H.colours(r) == f0["colours"], f"rank {r}"
        # the callbacks of precond 3 (tests/test_gpu_solve_dist_mg.py, tests/test_gpu_solve_dist_gmres.py), by their formulas
        def want(i):
            n, rs = i[I["iterations"]], i[I["restarts"]]
            if method == "bicgstab":
                return (6 * n + 2 + rs, 2 * (2 * (L - 2) + 7) * n, 3 * n + 2 + rs, 0)
            return (3 * n + 2 * (rs + 1) + rs + 2, (2 * (L - 2) + 7) * (n + rs + 1), rs + 2, 2 * n)
        for rk in ranks:
            assert e(rk)["calls"] == want(info) == rk[(method, rel_tol, 0)]["calls"]
            assert rk[(method, rel_tol, "jacobi")]["calls"] == want(jac)
            if (method, rel_tol) == ("bicgstab", 1e-8):      # the very first solve of the rig builds the hierarchy, as precond 3 does
                w = want(info)
                assert e(rk)["calls_first"] == (w[0], w[1] + L - 1, w[2] + L, 0)
            else:
                assert e(rk)["calls_first"] == want(info)


# ---- 4. mixed precision, ghosts that arrive late, the rule for the colours, collective decisions, refusals (two ranks) ----
def test_mixed_across_two_ranks(oracle):
    s, A, b = solve_ref_dist.global_system("pihna_kuhn", oracle)
    ranks = R.run("pihna_kuhn", 2)
    info, jac = _same_info(ranks, lambda rk: rk["mixed"]), _same_info(ranks, lambda rk: rk["mixed_jacobi"])
    xg = _gather(ranks, lambda rk: rk["mixed"], s.nv, s.xyz.shape[0])
    _ghosts_hold_owner_values(ranks, lambda rk: rk["mixed"], xg, s.nv)
    f = solve_ref.check_solution(A, b, xg.reshape(-1), s.nv, 2, 1e-8, extra_rel=ASSEMBLY_REL)
    print(f"mixed, world 2: {info[I['iterations']]} iterations (precond 3, mixed: {jac[I['iterations']]}), restarts {info[I['restarts']]}, residual "
          f"{f['residual_norm']:.3e} <= {f['bound']:.3e}")
    assert info[I["reason"]] == SOLVE_CONVERGED and info[I["matrix_bits"]] == 32
    assert jac[I["reason"]] == SOLVE_CONVERGED and info[I["iterations"]] <= jac[I["iterations"]]


def test_nothing_reads_a_ghost_before_it_arrives():
    """with one launch per colour the leading nodes of colour 0 run between exchange_begin and exchange_end, while the tail is NaN"""
    ranks = R.run("pihna_kuhn", 2)
    for rk in ranks:
        ref = rk[("bicgstab", 1e-10, 0)]
        assert np.all(np.isfinite(rk["nan"]["x"]))
        assert rk["nan"]["info"] == ref["info"] and rk["nan"]["info"][I["reason"]] == SOLVE_CONVERGED
        assert rk["nan"]["x"].tobytes() == ref["x"].tobytes()


def test_colours_go_and_come_with_the_partitioned_hierarchy(oracle):
    """the rule of DESIGN.md 7.2: a new plan drops the hierarchy and this rank's colours; the next solve with 6 builds both again"""
    ranks = R.run("pihna_kuhn", 2)
    _, H = Y.hierarchy("pihna_kuhn", 2, oracle)
    for r, rk in enumerate(ranks):
        ref = rk[("bicgstab", 1e-10, 1)]
        assert rk["nan"]["colours"] == H.colours(r)                 # built again behind the plan of the other communicator
        assert rk["after_plan"] == [ERR_STATE, ERR_STATE]
        assert rk["replanned"]["colours"] == H.colours(r)
        assert rk["replanned"]["x"].tobytes() == ref["x"].tobytes() and rk["replanned"]["info"] == ref["info"]
        n, rs, L = ref["info"][I["iterations"]], ref["info"][I["restarts"]], H.n_levels
        assert rk["replanned"]["calls"] == (6 * n + 2 + rs, 2 * (2 * (L - 2) + 7) * n + L - 1, 3 * n + 2 + rs + L, 0)


def test_collective_decisions_and_refusals(oracle):
    s, A, b = solve_ref_dist.global_system("pihna_kuhn", oracle)
    ranks = R.run("pihna_kuhn", 2)
    for rk in ranks:
        for key, word in (("refused_dist", "rdc_solve_dist_mg"), ("refused_solve", "ghost"), ("refused_mg_smoother1", "mg_smoother"),
                          ("refused_gmres_smoother1", "mg_smoother")):
            got = rk[key]
            assert got["code"] == ERR_UNSUPPORTED and word in got["message"], (key, got)
            assert got["calls"] == (0, 0, 0, 0) and got["untouched"], (key, got)
    info = _same_info(ranks, lambda rk: rk["singular"])
    assert info[I["reason"]] == SOLVE_BAD_DIAGONAL and info[I["bad_blocks"]] >= 1 and info[I["iterations"]] == 0
    assert all(rk["singular"]["owned_untouched"] for rk in ranks)
    assert _same_info(ranks, lambda rk: rk["restored"]) == _same_info(ranks, lambda rk: rk[("bicgstab", 1e-10, 1)])
    assert all(rk["restored"]["x"].tobytes() == rk[("bicgstab", 1e-10, 1)]["x"].tobytes() for rk in ranks)
    info = _same_info(ranks, lambda rk: rk["max_its"])
    assert info[I["reason"]] == SOLVE_MAX_ITS and info[I["iterations"]] == 3
    assert info[I["residual_norm"]] > 1e-10 * info[I["rhs_norm"]]


def test_refusals_on_one_partition():
    ctx, s, A, rhs, val = _open("hcc_hex")
    with ctx:
        comm = _world1_comm(s)
        xd = _dev(np.zeros(rhs.size))
        ctx.solve_dist(comm, xd.data_ptr(), precond=2, rhs_scale=s.rhs_scale)                  # uploads plan and peers
        p, info = SolveParams(1e-8, 0.0, s.rhs_scale, 100, GS), SolveInfo()
        with pytest.raises(RdcError, match="rdc_solve_dist_mg") as ei:
            ctx._ck(ctx._lib.rdc_solve_dist(ctx._h, C.byref(p), C.byref(comm.struct), 0, C.c_void_p(xd.data_ptr()), C.byref(info)))
        assert ei.value.code == ERR_UNSUPPORTED
        ctx.set_option("mg_smoother", 1)                                                       # precond 3 keeps its refusal
        xd = _dev(np.zeros(rhs.size))
        before = _counts(comm)
        for fn in (ctx.solve_dist, ctx.solve_dist_gmres):
            with pytest.raises(RdcError, match="mg_smoother") as ei:
                fn(comm, xd.data_ptr(), precond=MG, rhs_scale=s.rhs_scale)
            assert ei.value.code == ERR_UNSUPPORTED
        assert _counts(comm) == before and not xd.cpu().numpy().any()
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:
        xd = _dev(np.zeros(ctx.n_node * s.nv))
        with pytest.raises(RdcError, match="ghost") as ei:
            ctx.solve(xd.data_ptr(), precond=GS, rhs_scale=s.rhs_scale)
        assert ei.value.code == ERR_UNSUPPORTED
        with pytest.raises(RdcError) as ei:
            ctx.mg_apply(np.zeros(ctx.n_owned * s.nv))
        assert ei.value.code == ERR_UNSUPPORTED


# ---- 5. one cycle held to the extended-precision reference ----
def _assembled_in_rank_order(ranks, nv):
    """(Ap, b_p, counts): the global matrix of the rows the ranks assembled and downloaded, nodes in rank order"""
    counts = [rk["n_owned"] for rk in ranks]
    perm = np.concatenate([rk["node_global"][:rk["n_owned"]] for rk in ranks])
    pos = np.empty(perm.size, dtype=np.int64)
    pos[perm] = np.arange(perm.size)
    rows, rhs = [], []
    for rk in ranks:
        S = rk["system"]
        assert S["unchanged"], "the hook modified the CSR values or the rhs"
        col = (pos[rk["node_global"][S["col"] // nv]] * nv + S["col"] % nv).astype(np.int64)
        rows.append(sps.csr_matrix((S["val"], col, S["rp"]), shape=(rk["n_owned"] * nv, perm.size * nv)))
        rhs.append(S["rhs"])
    return sps.vstack(rows).tocsr(), np.concatenate(rhs), counts


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name,world", sorted(R.ARNOLDI_ON))
def test_one_cycle_against_reference(name, world, mixed):
    s = solve_ref_dist.case(name)
    ranks = R.run(name, world)
    nv = s.nv
    Ap, rhs_p, counts = _assembled_in_rank_order(ranks, nv)
    E = Y.EmulatedGs(Ap, nv, counts)
    M = solve_ref.precond_inverse(Ap, nv, 2)[0]
    if mixed:      # the iteration and the cycle's level 0 run on fl32(D^-1 A); the coarse levels stay those of the unrounded D^-1 A
        A32 = solve_ref_mixed.scaled_f32(Ap, nv, 2)
        assert np.all(np.isfinite(A32.data))
        G, C0, Cx = E.mixed(A32), Y.CycleLocal(E, Ap, op0=A32), Y.CycleLocal(E, Ap, op0=ld.scaled_f32_ld(Ap, nv))
        A32x = ld.Op.of_matrix(ld.scaled_f32_ld(Ap, nv))
        op = lambda v: A32 @ G.cycle(v)
        op_ld = lambda v: ld.Op.of_matrix(A32) @ C0.cycle(v)
        op_x = lambda v: A32x @ Cx.cycle(v)
    else:
        C0 = Y.CycleLocal(E, Ap)
        op = lambda v: M @ (Ap @ E.cycle(v))
        op_ld = lambda v: C0.levels[0]["op"] @ C0.cycle(v)
        op_x = None
    margin = ld.MARGIN_MIXED if mixed else ld.MARGIN
    for label in ("rhs", "random"):
        got = [rk[("arnoldi", mixed, label)] for rk in ranks]
        H = got[0]["H"]
        assert all(g["H"].tobytes() == H.tobytes() and g["V"].shape == (2, c * nv) for g, c in zip(got, counts))
        assert all(g["fuse0_same"] for g in got), "mg_gs_fuse 0 and 1 differ"
        V = np.concatenate([g["V"] for g in got], axis=1)
        assert np.all(np.isfinite(V)) and np.all(np.isfinite(H[:2, 0]))
        v0 = V[0].copy()                                       # the unit vector the device applied the operator to
        z = H[0, 0] * V[0] + H[1, 0] * V[1]                    # ... and what it got: D^-1 A M v0
        z_ld = op_ld(v0)
        noise = max(ld.rel_diff(op(v0), z_ld))
        noise32 = max(ld.rel_diff(op_x(v0), z_ld)) if mixed else 0.0
        bound = ld.bound(margin, noise, noise32)
        e2, einf = ld.rel_diff(z, z_ld)
        print(f"one cycle {name} world {world} mixed {int(mixed)} v0 {label}: error ({e2:.2e}, {einf:.2e}), noise {noise:.2e}, noise32 {noise32:.2e}, "
              f"error / noise {max(e2, einf) / max(noise, noise32, 16 * EPS):.2f}, bound {bound:.2e}; callbacks {got[0]['calls']}")
        assert bound <= ld.BOUND_CAP, (bound, noise, noise32)
        assert e2 <= bound and einf <= bound, (e2, einf, bound)
        # one cycle, one outer operator: 3 exchanges of the plan's size, 2 (L - 2) + 7 sized ones
        L = len(E.levels)
        assert all(g["calls"][0] == 3 and g["calls"][1] == 2 * (L - 2) + 7 for g in got)
