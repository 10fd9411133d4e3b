"""What the cached artefacts of the linear solve are worth after every kind of call ("validity of cached solve
artefacts"): one context on ripf_tet walks through a sequence of public calls, and after each step the four observers tell what
the context still vouches for --

  f32    csr_matvec_f32      ERR_INVALID without a usable fp32 copy
  mg     mg_level(1)         ERR_STATE without the values of a multigrid cycle
  ilu    ilu_factor          ERR_STATE without a factor
  gmres  gmres_stats         ERR_STATE without a GMRES solve

The expected pattern is written out below, step by step; nothing is read back from the library's own state."""
import numpy as np
import pytest

from solve_systems import _dev, _open
from rdcfes_amd import RdcError
from rdcfes_amd.context import (ERR_INVALID, ERR_STATE, PRECOND_BLOCK_JACOBI, PRECOND_ILU0, PRECOND_MULTIGRID, SOLVE_CONVERGED)

pytestmark = pytest.mark.gpu


def _observe(ctx, x):
    """(f32, mg, ilu, gmres): True = the observer answered, False = it refused with its documented code"""
    out = []
    for call, code in ((lambda: ctx.csr_matvec_f32(x), ERR_INVALID), (lambda: ctx.mg_level(1), ERR_STATE),
                       (ctx.ilu_factor, ERR_STATE), (ctx.gmres_stats, ERR_STATE)):
        try:
            call()
            out.append(True)
        except RdcError as e:
            assert e.code == code, str(e)
            out.append(False)
    return tuple(out)


def test_every_call_leaves_the_documented_artefacts_valid():
    ctx, s, A, rhs, _ = _open("ripf_tet")
    n = rhs.size
    x = np.linspace(-1.0, 1.0, ctx.n_node * s.nv)
    v = _dev(np.cos(np.arange(n)))

    def solve(**kw):
        xd = _dev(np.zeros(n))
        info = ctx.solve(xd.data_ptr(), rel_tol=1e-8, max_its=2000, **kw)
        assert info.reason == SOLVE_CONVERGED, (kw, info.reason)
        return info

    def refused_solve():
        with pytest.raises(RdcError) as e:
            ctx.solve(0, precond=PRECOND_MULTIGRID)   # a null x: refused behind the mesh check
        assert e.value.code == ERR_INVALID and "null argument" in str(e.value)

    def gmres_solve():
        ctx.set_option("solve_method", 1)
        solve(precond=PRECOND_BLOCK_JACOBI)
        ctx.set_option("solve_method", 0)

    def mixed_mg_solve():
        assert solve(precond=PRECOND_MULTIGRID, mixed=True).matrix_bits == 32

    #                                                                               f32    mg     ilu    gmres
    steps = [
        ("fresh", lambda: None,                                                     (False, False, False, False)),
        ("csr_scale_f32", ctx.csr_scale_f32,                                        (True, False, False, False)),
        ("FP64 multigrid solve", lambda: solve(precond=PRECOND_MULTIGRID),          (True, True, False, False)),
        ("block-Jacobi solve", lambda: solve(precond=PRECOND_BLOCK_JACOBI),         (True, False, False, False)),
        ("mg_apply", lambda: ctx.mg_apply_device(v.data_ptr(), _dev(np.zeros(n)).data_ptr()), (True, True, False, False)),
        ("ilu_apply", lambda: ctx.ilu_apply_device(v.data_ptr(), _dev(np.zeros(n)).data_ptr()), (True, False, True, False)),
        ("ILU(0) solve", lambda: solve(precond=PRECOND_ILU0),                       (True, False, True, False)),
        ("mixed multigrid solve", mixed_mg_solve,                                   (True, True, True, False)),
        ("solve refused for a null x", refused_solve,                               (True, False, True, False)),
        ("GMRES solve", gmres_solve,                                                (True, False, True, True)),
        ("second mesh_upload", lambda: s.upload(ctx),                               (False, False, False, False)),
    ]
    seen = []
    for name, call, _ in steps:
        call()
        ctx.synchronize()
        seen.append((name, _observe(ctx, x)))
        print(seen[-1])
    assert seen == [(name, want) for name, _, want in steps]
    ctx.close()
