"""rdc_solid_newton on the device against the numpy Newton of tests/solid_newton_ref.py (oracle assembly), on the two shipped solid
cases from the undeformed mesh: first residual, trajectory, end state, inexact Newton, step halving, the composition of the
existing calls, the preconditioners and methods, refusals and edge cases, and the host mirror's opt-in.

Between entry and exit of a solid_newton call nothing is downloaded: the tests read info and history, and download only afterwards."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import solid_newton_ref as N
import solve_systems
from rdcfes_amd import (AssemblyContext, RdcError, SolidMaterial, gmsh, inputs, partition, synth)
from rdcfes_amd.context import (ERR_INVALID, ERR_UNSUPPORTED, FIELD_ELEM_FIBRE, FIELD_UNDEFORMED_XYZ, NEWTON_CONVERGED_RESIDUAL, NEWTON_CONVERGED_STEP,
                                NEWTON_MAX_ITS, NEWTON_NOT_FINITE, PRECOND_BLOCK_JACOBI, PRECOND_ILU0, PRECOND_MULTIGRID)
from test_solid_newton_ref import HALVING_CAP

ROOT = Path(__file__).resolve().parent.parent
G = ROOT / "tests" / "golden"
pytestmark = pytest.mark.gpu
MARGIN = 64          # the project's margin over a measured floor (tests/test_gpu_mg_cycle.py)
TOL = 1e-10          # the project's parity bar
TIGHT = dict(max_nonlinear_iterations=10, require_reduction=False, relative_step_tolerance=0.0, relative_residual_tolerance=1e-8,
             absolute_residual_tolerance=1e-8)
CASES = [("cube", 0.1), ("cube", 1.0), ("hydrogel", 0.1)]


def _open(name, pt):
    s = N.at(N.system(name), pt)
    ctx = AssemblyContext(0)
    s.upload(ctx)
    return ctx, s


def _coords(ctx):
    return ctx.coords_tensor().cpu().numpy().copy()


def _device(name, pt, *, rel_tol, precond=PRECOND_BLOCK_JACOBI, mixed=False, options=(), x0=None, max_its=50000, **kw):
    """one solid_newton call on a fresh context -> dict(info, history, xyz, val, rhs); the downloads come after the call"""
    ctx, s = _open(name, pt)
    with ctx:
        for k, v in options:
            ctx.set_option(k, v)
        if x0 is not None:
            ctx.mesh_update_coords(x0)
        info = ctx.solid_newton(s.params, rel_tol=rel_tol, max_its=max_its, precond=precond, mixed=mixed, **kw)
        hist = ctx.solid_newton_history()
        val, rhs = ctx.csr_download()
        return dict(info=info, history=hist, xyz=_coords(ctx), val=val, rhs=rhs, s=s)


_REF = {}


def _ref(oracle, name, pt, linear, **kw):
    """the reference run, computed once per setting and left unchanged; linear: "exact" or a relative tolerance of solve_ref.bicgstab"""
    key = (name, pt, linear, tuple(sorted(kw.items())))
    if key not in _REF:
        s = N.at(N.system(name), pt)
        _REF[key] = N.newton(oracle, s, s.xyz, N.spsolve_linear if linear == "exact" else N.bicgstab_linear(linear), **kw)
    return _REF[key]


_TRAJ = {}


def _traj(name, pt):
    if (name, pt) not in _TRAJ:
        _TRAJ[(name, pt)] = _device(name, pt, rel_tol=1e-10, **TIGHT)
    return _TRAJ[(name, pt)]


@pytest.mark.parametrize("name", ["cube", "hydrogel"])
def test_first_residual(oracle, name):
    s = N.at(N.system(name), 0.1)
    _, R = N.assemble(oracle, s, s.xyz, jacobian=False)
    want = float(np.linalg.norm(R))
    d = _device(name, 0.1, rel_tol=1e-3, **dict(TIGHT, max_nonlinear_iterations=1))
    print(f"{name}: first residual {d['info'].first_residual!r}, oracle {want!r}, rel {abs(d['info'].first_residual - want) / want:.2e}")
    assert abs(d["info"].first_residual - want) <= TOL * want
    assert d["info"].nonlinear_iterations == 1 and d["info"].assemblies == 2 and d["info"].reason == NEWTON_MAX_ITS


@pytest.mark.parametrize("name,pt", CASES)
def test_trajectory_against_the_reference(oracle, name, pt):
    ref = _ref(oracle, name, pt, 1e-10, **TIGHT)
    exact = _ref(oracle, name, pt, "exact", **TIGHT)
    d = _traj(name, pt)
    info, (res, step, its, reason) = d["info"], d["history"]
    assert info.reason == ref["reason"] == NEWTON_CONVERGED_RESIDUAL and info.nonlinear_iterations == ref["nonlinear_iterations"]
    assert len(ref["residuals"]) == len(exact["residuals"])
    # nothing came back in between: one full assembly per iteration and the closing one, no trial
    assert info.assemblies == info.nonlinear_iterations + 1 and info.halvings == 0 and np.all(step == 1.0)
    assert info.linear_iterations == int(its.sum()) and np.all(reason == 0)
    got = list(res) + [info.last_residual]
    worst = 0.0
    for i, (g, r, e) in enumerate(zip(got, ref["residuals"], exact["residuals"])):
        floor = abs(r - e)
        ratio = abs(g - r) / floor if floor > 0 else float("nan")
        worst = max(worst, ratio) if floor > 0 else worst
        print(f"{name} {pt} it {i}: device {g:.10e} ref {r:.10e} exact {e:.10e} | dev-ref {abs(g - r):.2e} floor {floor:.2e} ratio {ratio:.2f} "
              f"| 1e-10 first {TOL * ref['first_residual']:.2e} | linear its {its[i] if i < len(its) else '-'}")
        assert abs(g - r) <= MARGIN * floor + TOL * ref["first_residual"], (i, g, r, floor)
    print(f"{name} {pt}: worst ratio to the floor {worst:.2f}")


@pytest.mark.parametrize("name,pt", CASES)
def test_end_state_checked_independently(oracle, name, pt):
    d = _traj(name, pt)
    info = d["info"]
    _, R = N.assemble(oracle, d["s"], d["xyz"], jacobian=False)
    rn = float(np.linalg.norm(R))
    print(f"{name} {pt}: last_residual {info.last_residual:.10e}, oracle at the returned coordinates {rn:.10e}")
    assert abs(info.last_residual - rn) <= TOL * info.first_residual
    assert info.reason == NEWTON_CONVERGED_RESIDUAL and (rn <= 1e-8 or rn <= 1e-8 * info.first_residual)


@pytest.mark.parametrize("name,pt", CASES)
def test_inexact_newton(oracle, name, pt):
    opt = N.shipped_options(name)
    lin = dict(rel_tol=opt.pop("rel_tol"), max_its=opt.pop("max_its"))
    assert lin["rel_tol"] == 1e-3 and opt["relative_step_tolerance"] == 1e-3
    s = N.at(N.system(name), pt)
    ref = N.newton(oracle, s, s.xyz, N.bicgstab_linear(lin["rel_tol"], max_its=lin["max_its"]), **opt)
    d = _device(name, pt, **lin, **opt)
    info, (res, step, its, reason) = d["info"], d["history"]
    print(f"{name} {pt}: reason {info.reason} (ref {ref['reason']}), iterations {info.nonlinear_iterations} (ref {ref['nonlinear_iterations']}), "
          f"linear {list(its)} (ref {ref['lin_its']}), residuals {[f'{r:.3e}' for r in res]} last {info.last_residual:.3e}")
    assert info.reason == ref["reason"] and info.nonlinear_iterations == ref["nonlinear_iterations"]
    assert its[0] == ref["lin_its"][0]
    if name == "cube":
        assert its[0] == 12
    assert info.assemblies == ref["assemblies"]


def test_halving(oracle):
    kw = dict(TIGHT, require_reduction=True, max_nonlinear_iterations=HALVING_CAP)
    ref = _ref(oracle, "cube", 1.5, 1e-10, **kw)
    assert min(ref["gaps"]) >= 1e-6 and ref["halvings"] >= 1        # the condition under which the branches must be the same
    d = _device("cube", 1.5, rel_tol=1e-10, **kw)
    info, (res, step, its, reason) = d["info"], d["history"]
    print(f"halving: steps {list(step)} (ref {ref['steps']}), halvings {info.halvings} (ref {ref['halvings']}), assemblies {info.assemblies} "
          f"(ref {ref['assemblies']}), residuals {[f'{r:.6e}' for r in res]} (ref {[f'{r:.6e}' for r in ref['residuals']]})")
    assert list(step) == ref["steps"] == [1.0, 0.25, 0.125]
    assert info.halvings == ref["halvings"] and info.assemblies == ref["assemblies"] and info.reason == ref["reason"] == NEWTON_MAX_ITS
    assert np.all(np.isfinite(res)) and np.isfinite(info.last_residual)


def _composed(ctx, s, *, rel_tol, max_its, precond, max_nonlinear_iterations, relative_residual_tolerance, absolute_residual_tolerance, **_):
    """the loop from Python with the existing calls, full step, stop by residual: what the library call replaces"""
    import torch
    u = _coords(ctx)
    delta = torch.zeros(u.size, dtype=torch.float64, device="cuda:0")
    out = dict(its=[], residuals=[], reason=None, n=0)
    it = 0
    while True:
        ctx.solid_assemble(s.params, True)
        _, rhs = ctx.csr_download(want_val=False)
        rn = float(np.linalg.norm(rhs))
        out["residuals"].append(rn)
        if rn <= absolute_residual_tolerance or rn <= relative_residual_tolerance * out["residuals"][0]:
            out["reason"] = NEWTON_CONVERGED_RESIDUAL
            break
        if it >= max_nonlinear_iterations:
            out["reason"] = NEWTON_MAX_ITS
            break
        delta.zero_()
        torch.cuda.synchronize()
        li = ctx.solve(delta.data_ptr(), rel_tol=rel_tol, max_its=max_its, precond=precond, rhs_scale=-1.0)
        out["its"].append(li.iterations)
        u = u + delta.cpu().numpy().reshape(u.shape)
        ctx.mesh_update_coords(u)
        it += 1
    out["n"], out["xyz"] = it, u
    return out


@pytest.mark.parametrize("name,pt", [("cube", 1.0), ("hydrogel", 0.1)])
def test_against_the_composition(oracle, name, pt):
    d = _traj(name, pt)
    ctx, s = _open(name, pt)
    with ctx:
        comp = _composed(ctx, s, rel_tol=1e-10, max_its=50000, precond=PRECOND_BLOCK_JACOBI, **TIGHT)
    info, (res, step, its, reason) = d["info"], d["history"]
    # Newton iterations and reasons are the same.  The linear iterations are printed, not compared: the solid assembly sums a node
    # block in the arrival order of its LDS atomics (rdc_solid_cl.hip) and the sides with hardware atomics (rdc_solid.hip), so two
    # assemblies of one state differ in the last bits and BiCGStab at 1e-10 takes a few iterations more or less from run to run
    print(f"{name} {pt}: linear iterations device {[int(v) for v in its]}, composed {comp['its']}")
    assert info.nonlinear_iterations == comp["n"] and info.reason == comp["reason"] and len(its) == len(comp["its"])
    assert np.all(reason == 0)
    ref = _ref(oracle, name, pt, 1e-10, **TIGHT)
    exact = _ref(oracle, name, pt, "exact", **TIGHT)
    floor = float(np.linalg.norm(ref["xyz"] - exact["xyz"]))
    dev = float(np.linalg.norm(d["xyz"] - comp["xyz"]))
    un = float(np.linalg.norm(d["xyz"]))
    print(f"{name} {pt}: |u_device - u_composed| {dev:.3e}, floor {floor:.3e}, 1e-10 |u| {TOL * un:.3e}")
    assert dev <= MARGIN * floor + TOL * un
    # the context holds the assembly at the returned coordinates
    A, R = N.assemble(oracle, d["s"], d["xyz"])
    assert np.linalg.norm(d["val"] - A.data) <= TOL * np.linalg.norm(A.data)
    assert np.linalg.norm(d["rhs"] - R) <= TOL * max(np.linalg.norm(R), info.first_residual)


@pytest.mark.parametrize("what", ["multigrid", "ilu0", "mixed", "gmres"])
def test_preconditioners_and_methods_pass_through(oracle, what):
    ref = _ref(oracle, "cube", 0.1, 1e-10, **TIGHT)
    kw = dict(multigrid=dict(precond=PRECOND_MULTIGRID), ilu0=dict(precond=PRECOND_ILU0), mixed=dict(mixed=True),
              gmres=dict(options=(("solve_method", 1),)))[what]
    d = _device("cube", 0.1, rel_tol=1e-10, **kw, **TIGHT)
    info, (res, step, its, reason) = d["info"], d["history"]
    print(f"{what}: iterations {info.nonlinear_iterations}, linear {list(its)}, residuals {[f'{r:.3e}' for r in res]} last {info.last_residual:.3e}")
    assert info.reason == NEWTON_CONVERGED_RESIDUAL and info.nonlinear_iterations == ref["nonlinear_iterations"]
    assert info.linear_iterations == int(its.sum()) and len(its) == info.nonlinear_iterations and np.all(reason == 0)
    assert info.last_residual <= max(1e-8, 1e-8 * info.first_residual)


def test_refusals():
    # a ghosted context with 3 unknowns per node: rank 0 of a two-way split, everything the assembly needs set
    conn, xyz = synth.kuhn_tet_mesh(8, order="random")
    part = partition.partition_rcb(xyz[conn.astype(np.int64)].mean(axis=1), 2)
    lp = partition.build_local(conn, xyz, part, 0, 2, owner=partition.node_owners(conn, part, xyz.shape[0], 2))
    assert 0 < lp.n_owned < lp.xyz.shape[0]
    opt = dict(TIGHT, rel_tol=1e-3, max_its=100)
    sp = N.system("cube").params
    with AssemblyContext(0) as ctx:
        ctx.mesh_upload(4, lp.conn, lp.xyz, 3, n_owned=lp.n_owned)
        ctx.field_upload(FIELD_UNDEFORMED_XYZ, lp.xyz)
        ctx.field_upload(FIELD_ELEM_FIBRE, np.tile([0.0, 0.0, 1.0], (lp.conn.shape[0], 1)))
        ctx.solid_set_materials(np.zeros(lp.conn.shape[0], dtype=np.int32), [SolidMaterial(1.0e3, 0.3, 0.0, (0.0, 0.0, 0.0))])
        with pytest.raises(RdcError) as ei:
            ctx.solid_newton(sp, **opt)
        assert ei.value.code == ERR_UNSUPPORTED and "ghost" in str(ei.value)
        assert _coords(ctx).tobytes() == np.ascontiguousarray(lp.xyz).tobytes()
    # 5 unknowns per node
    with AssemblyContext(0) as ctx:
        solve_systems.get("pihna_kuhn").upload(ctx)
        with pytest.raises(RdcError) as ei:
            ctx.solid_newton(sp, **opt)
        assert ei.value.code == ERR_INVALID
    # parameters
    ctx, s = _open("cube", 0.1)
    with ctx:
        for bad in (dict(max_nonlinear_iterations=0), dict(max_nonlinear_iterations=1001), dict(relative_step_tolerance=float("nan")),
                    dict(absolute_residual_tolerance=-1.0), dict(precond=17), dict(max_its=0)):
            with pytest.raises(RdcError) as ei:
                ctx.solid_newton(s.params, **dict(opt, **bad))
            assert ei.value.code == ERR_INVALID, bad
        assert _coords(ctx).tobytes() == np.ascontiguousarray(s.xyz).tobytes()


def test_a_converged_start_is_left_alone():
    ctx, s = _open("cube", 0.1)
    with ctx:
        kw = dict(TIGHT, rel_tol=1e-10, max_its=50000)
        first = ctx.solid_newton(s.params, **kw)
        assert first.reason == NEWTON_CONVERGED_RESIDUAL and first.nonlinear_iterations >= 1
        before = _coords(ctx)
        again = ctx.solid_newton(s.params, **dict(kw, relative_residual_tolerance=0.0, absolute_residual_tolerance=2.0 * first.last_residual))
        assert again.reason == NEWTON_CONVERGED_RESIDUAL and again.nonlinear_iterations == 0 and again.assemblies == 1
        # (two assemblies of one state agree to rounding, not bitwise: the atomics of the solid kernels arrive in any order)
        assert again.linear_iterations == 0 and again.first_residual == again.last_residual
        assert abs(again.last_residual - first.last_residual) <= TOL * first.first_residual
        assert _coords(ctx).tobytes() == before.tobytes()
        assert len(ctx.solid_newton_history()[0]) == 0


def test_a_nan_coordinate_is_reported_not_propagated():
    ctx, s = _open("cube", 0.1)
    with ctx:
        x0 = np.ascontiguousarray(s.xyz).copy()
        x0[17, 2] = np.nan
        ctx.mesh_update_coords(x0)
        info = ctx.solid_newton(s.params, rel_tol=1e-3, max_its=100, **TIGHT)
        assert info.reason == NEWTON_NOT_FINITE and info.nonlinear_iterations == 0 and info.assemblies == 1 and info.linear_iterations == 0
        assert not np.isfinite(info.first_residual)
        assert _coords(ctx).tobytes() == x0.tobytes()


def test_stop_by_step():
    """the shipped relative_step_tolerance with a tight linear solve: the cube at 0.1 stops by step after 2 iterations, 3 assemblies"""
    d = _device("cube", 0.1, rel_tol=1e-10, **dict(TIGHT, relative_step_tolerance=1e-3))
    info = d["info"]
    assert info.reason == NEWTON_CONVERGED_STEP and info.nonlinear_iterations == 2 and info.assemblies == 3
    assert info.last_step_norm <= 1e-3 * info.last_solution_norm
    assert abs(info.last_solution_norm - np.linalg.norm(d["xyz"])) <= TOL * info.last_solution_norm


@pytest.fixture(scope="module")
def driver():
    from rdcfes_amd import build
    lib = build.build(verbose=False)
    out = ROOT / "tests" / "_build" / "solid_newton_mirror_driver"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "solid_newton_mirror_driver.cpp"
    hdr = ROOT / "rdcfes_amd" / "host" / "rdc_host.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime, lib.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", str(src), "-o", str(out), f"-L{lib.parent}", "-lrdc_assembly",
                        f"-Wl,-rpath,{lib.parent}"], check=True)
    return out


def test_host_mirror_opt_in(oracle, driver, tmp_path):
    """SolidSystem::run_solver() of the host mirror on the shipped cube, one loading step, with solve_on_device and without.
    The two paths differ in their linear solver: the host stand-in bicgstab_ilu0 stops on the plain residual ||b - A x|| <= tol ||b||,
    the device on the block-Jacobi-preconditioned one.  With the penalty of 1e8 next to a stiffness of order 1e3 the plain residual
    bounds the error of the update only through 1 / lambda_min(J), several orders more loosely than the preconditioned one, so the
    linear tolerance of this test is 1e-13 (capped at 2000 iterations, RDC_SOLVE_MAX_ITS being used as it is) and the relative
    residual tolerance 1e-10, which the cube meets after 3 iterations with a factor of 45 and more to either side (||R|| = 8.9e-3,
    then 2.1e-6, against 2.0e-4: tests/test_solid_newton_ref.py pins the first): the last update is then 1.8e-6 long, and what a
    linear solver leaves of it lies far below the bound on the positions, which is that of the trajectory test."""
    mesh = gmsh.read_msh2(G / "solid_uniaxial_compression_cube.msh")
    setup = inputs.read_solid_input(G / "solid_uniaxial_compression_input.dat")
    L = []
    for bc, disp in sorted(setup.bcs.items()):
        L.append(f"point BC/{bc}/displacement " + " ".join("nan" if np.isnan(v) else repr(float(v)) for v in disp))
    L.append("string BCs " + " ".join(str(b) for b in sorted(setup.bcs)))
    L.append(f"real BCs/displacement_penalty {setup.penalty!r}")
    for m, mat in setup.materials.items():
        h = f"material/{m}/Hyperelastic/"
        L += [f"real {h}Young {mat.Young!r}", f"real {h}Poisson {mat.Poisson!r}", f"real {h}FibreStiffness {mat.FibreStiffness!r}"]
        L += [f"real {h}VolumetricStretchRatio/rate_{d} {mat.rate[d]!r}" for d in range(3)]
    L += [f"real loading_step {setup.loading_step!r}", "bool solver/quiet true", "int solver/nonlinear/max_nonlinear_iterations 10",
          "real solver/nonlinear/relative_step_tolerance 0.0", "real solver/nonlinear/relative_residual_tolerance 1e-10",
          "real solver/nonlinear/absolute_residual_tolerance 1e-8", "bool solver/nonlinear/require_reduction false",
          "int solver/linear/max_linear_iterations 2000", "real solver/linear/initial_linear_tolerance 1e-13"]
    (tmp_path / "params.txt").write_text("\n".join(L) + "\n")
    mesh.conn.astype(np.uint32).tofile(tmp_path / "conn.bin")
    mesh.xyz.astype(np.float64).tofile(tmp_path / "xyz.bin")
    mesh.subdomain.astype(np.int32).tofile(tmp_path / "subdomain.bin")
    sides = []
    for bid in np.unique(mesh.face_tag):
        e, sd = mesh.sides_with_boundary_id(int(bid))
        sides += [(int(a), int(b), int(bid)) for a, b in zip(e, sd)]
    np.array(sides, dtype=np.int64).tofile(tmp_path / "sides.bin")
    np.tile([0.0, 0.0, 1.0], (mesh.conn.shape[0], 1)).astype(np.float64).tofile(tmp_path / "fibre.bin")
    out = {}
    for tag, on in (("host", 0), ("device", 1)):
        r = subprocess.run([str(driver), str(tmp_path), "8", str(on), tag], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        w = (tmp_path / f"log_{tag}.txt").read_text().split()
        out[tag] = dict(zip(w[0::2], w[1::2]), xyz=np.fromfile(tmp_path / f"sol_{tag}.bin").reshape(-1, 3))
    print({k: {a: b for a, b in v.items() if a != "xyz"} for k, v in out.items()})
    assert int(out["host"]["converged"]) == int(out["device"]["converged"]) == 1
    assert int(out["host"]["newton_iterations"]) == int(out["device"]["newton_iterations"]) == 3
    assert int(out["device"]["assemblies"]) == 4
    ref = _ref(oracle, "cube", 0.1, 1e-10, **TIGHT)
    exact = _ref(oracle, "cube", 0.1, "exact", **TIGHT)
    floor = float(np.linalg.norm(ref["xyz"] - exact["xyz"]))
    dev = float(np.linalg.norm(out["host"]["xyz"] - out["device"]["xyz"]))
    un = float(np.linalg.norm(out["device"]["xyz"]))
    print(f"mirror: |u_host - u_device| {dev:.3e}, floor {floor:.3e}, 1e-10 |u| {TOL * un:.3e}")
    assert dev <= MARGIN * floor + TOL * un
    assert np.linalg.norm(out["device"]["xyz"] - mesh.xyz) > 0.02       # the mesh did move
