"""ONE application of the device multigrid cycle (rdc_solve_mg_apply) and the coarse matrices it is built on
(rdc_solve_mg_level_download) against the extended-precision reference of tests/solve_ref_mg_ld.py, built from the system
downloaded from the GPU.  A cycle that is subtly wrong still converges, within the iteration slack of tests/test_gpu_solve_mg.py
and tests/test_gpu_solve_mg_gs.py (tests/test_solve_ref_mg_ld.py has the record); compared directly it has seven orders of
magnitude less room.

Bound of the cycle: ||z_gpu - z_ld|| <= MARGIN x max(noise, 16 eps) ||z_ld|| in the 2-norm and the max norm; noise is what numpy's
FP64 evaluation of the same cycle differs from the reference by on the same system and inputs (mixed: also noise32, what one-ulp
differences of the fp32 copy of D^-1 A do) -- measured on the reference, never on the device result.  The device uses fma, a
16-lane butterfly and a Gauss-Jordan inverse of its own, so it is not numpy's evaluation; its error / noise measured on an MI355X,
largest over the inputs of a case (Jacobi / Gauss-Seidel smoother):

  system          FP64 cycle      mixed cycle     D_l^-1 against np.linalg.inv, levels 0 / 1 / 2
  pihna_kuhn      1.65 / 1.46     4.04 / 5.65     1.89 / 0.31 / 0.41
  hcc_hex         0.40 / 0.44     1.00 / 1.00     0.54 / 0.19 / 0.11
  solid_cube      0.10 / 0.32     0.11 / 0.30     0.17 / 0.21 / 0.24
  pihna_hub       0.08 / 0.12     0.79 / 0.78     0.33 / 0.31 / 0.25
  pihna_hydrogel  4.15 / 13.71    3.31 / 0.90     67.98 / 0.40 / 0.27
  ripf_tet                           - / 0.06
  (errors 2e-16 .. 3e-10; the hydrogel blocks have condition numbers up to 2e13, and the Gauss-Jordan inverse of the device
  is then off by 2e-11 where LAPACK's is by 7e-11 at worst, but not on the same nodes)

MARGIN = 128, MARGIN_MIXED = 64 and MARGIN_INV = 1024 (tests/solve_ref_mg_ld.py) are the next power of two at or above 8 x the
largest of these: 8 x 13.71, 8 x 5.65, 8 x 67.98 (MARGIN_INV is at its cap of 1024).
Every case must also keep its bound below 1e-6 (solve_ref_mg_ld.BOUND_CAP): that is a condition, not a measurement.

Bounds of the coarse values: the standard bound of a sum formed from 0.0 in list order without contraction, per entry, each level
from the DEVICE's own values of the level above (level 1: from its D^-1 and the CSR values), so that an ill-conditioned D^-1 does
not enter: gamma(nvar + m) sum |D^-1||A| for level 1, gamma(m) sum |summand| below, gamma(k) = k eps / (1 - k eps), m = summands."""
import numpy as np
import pytest

import solve_ref_mg
import solve_ref_mg_gs
import solve_ref_mg_ld as ld
import solve_ref_mixed
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import RdcError
from rdcfes_amd.context import ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED, PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, SOLVE_CONVERGED

pytestmark = pytest.mark.gpu
FIVE = ["pihna_kuhn", "hcc_hex", "solid_cube", "pihna_hub", "pihna_hydrogel"]
EPS = ld.EPS
_REF = {}


class _Ref:
    """the numpy hierarchies and the extended-precision cycles of one downloaded system, each built when first asked for"""

    def __init__(self, A, b, nv):
        self.A, self.b, self.nv = A, b, nv
        self.base = solve_ref_mg.Hierarchy(A, nv)
        self._H, self._C, self._noise = {0: self.base}, {}, {}
        self.A32 = solve_ref_mixed.scaled_f32(A, nv, 2)
        assert np.all(np.isfinite(self.A32.data))      # else the device would fall back to the FP64 form

    def H(self, smoother, mixed=False):
        if smoother not in self._H:
            self._H[smoother] = solve_ref_mg_gs.Hierarchy(self.A, self.nv, base=self.base)
        return ld.mixed_hierarchy(self._H[smoother], self.A32) if mixed else self._H[smoother]

    def C(self, smoother, mixed=False):
        if (smoother, mixed) not in self._C:
            self._C[(smoother, mixed)] = ld.Cycle(self.H(smoother), self.A, op0=self.A32 if mixed else None)
        return self._C[(smoother, mixed)]

    def inputs(self, name):
        n = self.b.size
        unit = np.zeros(n)
        unit[-1] = 1.0                                    # the last unknown: the tail of every grid
        out = ld.probe_vectors(n, self.b) + [unit]
        if name == "pihna_hub":                          # ... and the node that owns the row of 740 blocks
            bptr = self.base.levels[0]["bptr"]
            hub = int(np.argmax(np.diff(bptr)))
            assert bptr[hub + 1] - bptr[hub] >= 740
            unit = np.zeros(n)
            unit[hub * self.nv] = 1.0
            out.append(unit)
        return out

    def noise(self, name, smoother, mixed):
        """(noise, noise32, [z_ld per input]) of a case; noise over both norms and every input"""
        key = (smoother, mixed)
        if key not in self._noise:
            C, vs = self.C(smoother, mixed), self.inputs(name)
            zs = [C.cycle(v) for v in vs]
            H = self.H(smoother, mixed)
            noise = max(max(ld.rel_diff(H.cycle(v), z)) for v, z in zip(vs, zs))
            noise32 = 0.0
            if mixed:
                Cx = ld.Cycle(self.H(smoother), self.A, op0=ld.scaled_f32_ld(self.A, self.nv))
                noise32 = max(max(ld.rel_diff(Cx.cycle(v), z)) for v, z in zip(vs, zs))
            self._noise[key] = (noise, noise32, zs)
        return self._noise[key]


def _ref(name, A, b, nv, val):
    """The reference of the values THIS context assembled: two contexts differ in the last bits (the assembly adds with atomics),
    and the noise is that of the system at hand.  Kept for the next test of the system should it download the same bytes."""
    if name not in _REF or _REF[name][0] != val.tobytes():
        _REF[name] = (val.tobytes(), _Ref(A, b, nv))
    return _REF[name][1]


def _values_tensor(ctx, size):
    """the CSR values of a context as a device tensor (no copy)"""
    import torch
    vptr, _ = ctx.csr_values_device_ptr()

    class _V:
        pass
    view = _V()
    view.__cuda_array_interface__ = {"shape": (size,), "typestr": "<f8", "data": (vptr, False), "version": 2, "strides": None}
    return torch.as_tensor(view, device="cuda:0")


def _raises(code, fn, match=None):
    with pytest.raises(RdcError, match=match) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return ei.value


CASES = [(n, sm, mx) for n in FIVE for sm in (0, 1) for mx in (False, True)] + [("ripf_tet", 1, True)]


@pytest.mark.parametrize("name,smoother,mixed", CASES)
def test_cycle_against_reference(name, smoother, mixed):
    """ripf_tet: level 0 itself is below the fused size, so the fp32 Gauss-Seidel sweep of level 0 runs in one workgroup"""
    ctx, s, A, rhs, val = _open(name)
    R = _ref(name, A, s.rhs_scale * rhs, s.nv, val)
    noise, noise32, zs = R.noise(name, smoother, mixed)
    bound = ld.bound(ld.MARGIN_MIXED if mixed else ld.MARGIN, noise, noise32)
    with ctx:
        ctx.set_option("mg_smoother", smoother)
        got = [ctx.mg_apply(v, mixed=mixed) for v in R.inputs(name)]
        if mixed:
            ctx.csr_matvec_f32(R.inputs(name)[0])          # the call left a usable fp32 copy: the cycle ran on it
        levels = ctx.mg_levels()
        _unchanged(ctx, val, rhs)
    errs = [ld.rel_diff(z, z_ld) for z, z_ld in zip(got, zs)]
    worst = max(max(e) for e in errs)
    print(f"cycle {name} smoother {smoother} mixed {int(mixed)}: error {worst:.2e}, noise {noise:.2e}, noise32 {noise32:.2e}, "
          f"error / noise {worst / max(noise, noise32, 16 * EPS):.2f}, bound {bound:.2e}; per input (2-norm, max norm) "
          + ", ".join(f"({a:.1e}, {b:.1e})" for a, b in errs))
    assert levels == R.base.level_sizes()
    assert bound <= ld.BOUND_CAP, (bound, noise, noise32)
    for z, (e2, einf) in zip(got, errs):
        assert np.all(np.isfinite(z))
        assert e2 <= bound and einf <= bound, (e2, einf, bound)


def _node_blocks(val, bptr, nv):
    """[blocks][nv][nv] from the node-block layout [var a][block k][var b] per node"""
    out = np.empty((int(bptr[-1]), nv, nv))
    for n in range(bptr.size - 1):
        b0, b1 = int(bptr[n]), int(bptr[n + 1])
        out[b0:b1] = val[nv * nv * b0:nv * nv * b1].reshape(nv, b1 - b0, nv).transpose(1, 0, 2)
    return out


def _gamma(k):
    return k * EPS / (1.0 - k * EPS)


def _check_inverse(what, X_gpu, blocks):
    """D_l^-1 per node against the extended-precision inverse of the same block, by the error np.linalg.inv makes on it"""
    nv = blocks.shape[1]
    X = ld.newton_inverse(blocks)
    fro = lambda M: np.sqrt((M * M).sum(axis=(1, 2))).astype(np.float64)
    e_gpu = fro(X_gpu.astype(ld.LD) - X) / fro(X)
    e_np = fro(np.linalg.inv(blocks).astype(ld.LD) - X) / fro(X)
    ratio = e_gpu / np.maximum(e_np, nv * EPS)
    print(f"{what}: D^-1 error / max(error of np.linalg.inv, nvar eps) at most {ratio.max():.2f} (errors up to {e_gpu.max():.1e} / {e_np.max():.1e})")
    assert np.all(np.isfinite(X_gpu)) and ratio.max() <= ld.MARGIN_INV <= ld.MARGIN_INV_CAP


@pytest.mark.parametrize("name", FIVE)
def test_coarse_values(name):
    ctx, s, A, rhs, val = _open(name)
    R = _ref(name, A, s.rhs_scale * rhs, s.nv, val)
    H, nv = R.base, s.nv
    x = ld.probe_vectors(rhs.size, rhs)[0]
    with ctx:
        _raises(ERR_STATE, lambda: ctx.mg_level(0))
        ctx.mg_apply(x)
        sizes = ctx.mg_levels()
        assert sizes == H.level_sizes() and len(sizes) >= 3
        got = [ctx.mg_level(l) for l in range(len(sizes))]
        if name == "pihna_kuhn":      # the Galerkin products read the FP64 values whatever the cycle streams
            ctx.mg_apply(x, mixed=True)
            for l in range(1, len(sizes)):
                v32, d32 = ctx.mg_level(l)
                assert v32.tobytes() == got[l][0].tobytes() and d32.tobytes() == got[l][1].tobytes()
    bptr, bcol, a0 = solve_ref_mg.block_pattern(A, nv)
    assert got[0][0] is None
    _check_inverse(f"{name} level 0", got[0][1], ld.diag_of(bptr, bcol, a0))
    rows = np.repeat(np.arange(bptr.size - 1), np.diff(bptr))
    dinv = got[0][1][rows]
    summands, sizes_abs = dinv.astype(ld.LD) @ a0.astype(ld.LD), np.abs(dinv) @ np.abs(a0)
    for l in range(1, len(sizes)):
        lv = H.levels[l]
        v, d = got[l]
        assert v.size == sizes[l][1] * nv * nv and d.shape == (sizes[l][0], nv, nv) and not np.any(np.isnan(v))
        blocks = _node_blocks(v, lv["bptr"], nv)
        cptr, cidx = ld.galerkin_lists(H, l)
        m = np.diff(cptr)[:, None, None]
        want, scale = ld.galerkin(summands, cptr, cidx), ld.galerkin(sizes_abs, cptr, cidx).astype(np.float64)
        err = np.abs(blocks.astype(ld.LD) - want).astype(np.float64)
        limit = _gamma((nv if l == 1 else 0) + m) * scale
        print(f"{name} level {l}: {sizes[l]} nodes / blocks, up to {int(m.max())} summands; largest |err| / bound {np.max(err / np.where(limit > 0, limit, 1.0)):.3f}")
        assert np.all(err <= limit), f"level {l}: {np.count_nonzero(err > limit)} entries off"
        _check_inverse(f"{name} level {l}", d, ld.diag_of(lv["bptr"], lv["bcol"], blocks))
        summands, sizes_abs = blocks.astype(ld.LD), np.abs(blocks)     # the next level sums the device's own values


def _solve(ctx, n, **kw):
    xd = _dev(np.zeros(n))
    info = ctx.solve(xd.data_ptr(), max_its=2000, **kw)
    return info, xd.cpu().numpy()


def _same(a, b):
    return all(getattr(a, f) == getattr(b, f) for f in ("reason", "iterations", "restarts", "bad_blocks", "rhs_norm", "residual_norm",
                                                        "plain_rhs_norm", "plain_residual_norm", "matrix_bits"))


@pytest.mark.parametrize("smoother", [0, 1])
@pytest.mark.parametrize("name", ["pihna_hydrogel", "hcc_hex"])
def test_cycle_is_stateless_and_the_solve_is_undisturbed(name, smoother):
    ctx, s, A, rhs, val = _open(name)
    R = _ref(name, A, s.rhs_scale * rhs, s.nv, val)
    noise, _, _ = R.noise(name, smoother, False)
    bound = ld.bound(ld.MARGIN, noise)
    u, v = ld.probe_vectors(rhs.size, rhs)[:2]
    kw = dict(rel_tol=1e-10, precond=PRECOND_MULTIGRID, rhs_scale=s.rhs_scale)
    with ctx:
        ctx.set_option("mg_smoother", smoother)
        i0, x0 = _solve(ctx, rhs.size, **kw)
        zu = ctx.mg_apply(u)                                # right after a solve
        zv = ctx.mg_apply(v)
        zu2 = ctx.mg_apply(u)
        assert zu.tobytes() == zu2.tobytes(), "a coarse vector leaks from one cycle into the next"
        if smoother == 1:
            ctx.set_option("mg_gs_fuse", 0)
            assert ctx.mg_apply(u).tobytes() == zu.tobytes(), "one launch per colour differs from one launch per sweep"
            ctx.set_option("mg_gs_fuse", 1)
        zl = ctx.mg_apply(2.0 * u - 3.0 * v)
        i1, x1 = _solve(ctx, rhs.size, **kw)
        _unchanged(ctx, val, rhs)
    assert i0.reason == SOLVE_CONVERGED and _same(i0, i1) and x0.tobytes() == x1.tobytes(), "the probes changed what a solve returns"
    # M is linear: each of the three results is within bound of its exact value, so the combination is within the sum
    nrm = np.linalg.norm
    lin = nrm(zl - (2.0 * zu - 3.0 * zv))
    print(f"{name} smoother {smoother}: ||M(2u - 3v) - (2 Mu - 3 Mv)|| = {lin:.2e}, bound {bound * (nrm(zl) + 2.0 * nrm(zu) + 3.0 * nrm(zv)):.2e}")
    assert lin <= bound * (nrm(zl) + 2.0 * nrm(zu) + 3.0 * nrm(zv))
    fresh, _, _, _, val2 = _open(name)
    with fresh:
        import torch
        _values_tensor(fresh, val.size).copy_(_dev(val))    # two assemblies differ in the last bits: the same values for both
        torch.cuda.synchronize()
        fresh.set_option("mg_smoother", smoother)
        assert fresh.mg_apply(u).tobytes() == zu.tobytes(), "an apply behind a solve differs from an apply on a fresh context"


def test_refusals():
    import torch
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:
        for smoother in (0, 1):
            ctx.set_option("mg_smoother", smoother)
            for mixed in (False, True):
                _raises(ERR_UNSUPPORTED, lambda: ctx.mg_apply(np.zeros(rhs.size), mixed=mixed), match="ghost")
        _raises(ERR_STATE, lambda: ctx.mg_level(0))
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size
    x = ld.probe_vectors(n, rhs)[0]
    with ctx:
        raw = lambda level, v=None, d=None: ctx._lib.rdc_solve_mg_level_download(ctx._h, level, v, d)
        _raises(ERR_STATE, lambda: ctx.mg_level(0))         # no apply, no multigrid solve
        assert raw(0) == ERR_STATE
        xd = _dev(x)
        _raises(ERR_INVALID, lambda: ctx.mg_apply_device(0, xd.data_ptr()))
        _raises(ERR_INVALID, lambda: ctx.mg_apply_device(xd.data_ptr(), 0))
        z = ctx.mg_apply(x)
        levels = ctx.mg_levels()
        built = [ctx.mg_level(l) for l in range(len(levels))]
        for bad in (-1, len(levels), 99):
            _raises(ERR_INVALID, lambda: ctx.mg_level(bad))
            assert raw(bad) == ERR_INVALID
        from rdcfes_amd.context import _dp
        assert raw(0, _dp(np.empty(levels[0][1] * 25))) == ERR_INVALID      # level 0 is the matrix itself: no values
        assert raw(1) == 0                                  # both pointers null: nothing to copy
        ctx.csr_scale_f32()                                 # writes over D^-1
        _raises(ERR_STATE, lambda: ctx.mg_level(1))
        _solve(ctx, n, rel_tol=1e-8, precond=PRECOND_MULTIGRID)
        for l, (v0, d0) in enumerate(built):                # a multigrid solve builds what the apply built
            v1, d1 = ctx.mg_level(l)
            assert d1.tobytes() == d0.tobytes() and (l == 0 or v1.tobytes() == v0.tobytes())
        _solve(ctx, n, rel_tol=1e-8, precond=PRECOND_BLOCK_JACOBI)
        _raises(ERR_STATE, lambda: ctx.mg_level(1))
        # a zeroed diagonal block: refused with the count, the output vector untouched
        val_d = _values_tensor(ctx, val.size)
        rp, col = ctx.csr_pattern()
        node = 11
        idx = np.concatenate([np.arange(rp[node * 5 + a], rp[node * 5 + a + 1])[col[rp[node * 5 + a]:rp[node * 5 + a + 1]] // 5 == node]
                              for a in range(5)])
        assert idx.size == 25
        keep = val_d.clone()
        val_d[torch.from_numpy(idx).to("cuda:0")] = 0.0
        for smoother in (0, 1):
            ctx.set_option("mg_smoother", smoother)
            for mixed in (False, True):
                y0 = np.random.default_rng(2).uniform(size=n)
                yd = _dev(y0)
                torch.cuda.synchronize()
                e = _raises(ERR_INVALID, lambda: ctx.mg_apply_device(xd.data_ptr(), yd.data_ptr(), mixed), match="not invertible")
                assert any(ch.isdigit() and ch != "0" for ch in str(e))
                assert yd.cpu().numpy().tobytes() == y0.tobytes()
        val_d.copy_(keep)
        torch.cuda.synchronize()
        ctx.set_option("mg_smoother", 0)
        assert ctx.mg_apply(x).tobytes() == z.tobytes()
