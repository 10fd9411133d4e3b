"""tests/solve_ref_mg_ld.py -- the extended-precision evaluation of the multigrid cycle, the reference of tests/test_gpu_mg_cycle.py --
pinned on the CPU on oracle-assembled systems:

(a) noise: what the numpy FP64 cycle differs from it by, per system and smoother (at most 1e-9; the figures printed here are the
    record in DESIGN.md 7.2);
(b) noise32: what one-ulp differences of the fp32 copy of D^-1 A do to the mixed cycle;
(c) the record that a comparison of ONE cycle sees faults which the assertions on a converged solve (tests/test_gpu_solve_mg.py,
    tests/test_gpu_solve_mg_gs.py: iterations <= yardstick + 2) cannot: four faults a device cycle could have, each a small
    override of the numpy hierarchy, move the cycle by at least 1000 x the bound of the GPU test, and three of them leave both
    iteration counts (rel_tol 1e-8 and 1e-10) within yardstick + 2."""
import copy

import numpy as np
import pytest
import scipy.sparse as sps

import solve_ref
import solve_ref_mg
import solve_ref_mg_gs
import solve_ref_mg_ld as ld
import solve_ref_mixed
import solve_systems
from solve_ref_mg import COARSEST_SWEEPS

SYSTEMS = ["pihna_kuhn", "hcc_hex", "solid_cube", "pihna_hub", "pihna_hydrogel", "ripf_tet"]
SMOOTHERS = {0: "Jacobi", 1: "GS"}
_CACHE = {}


def _system(oracle, name):
    """(system, A, b, {smoother: numpy hierarchy}, {smoother: extended-precision cycle}), once per system"""
    if name not in _CACHE:
        s = solve_systems.get(name)
        rp, col, val, rhs = s.oracle_assemble(oracle)
        A = sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size))
        base = solve_ref_mg.Hierarchy(A, s.nv)
        H = {0: base, 1: solve_ref_mg_gs.Hierarchy(A, s.nv, base=base)}
        _CACHE[name] = (s, A, s.rhs_scale * rhs, H, {k: ld.Cycle(h, A) for k, h in H.items()})
    return _CACHE[name]


def test_the_extended_format_has_a_64_bit_mantissa():
    assert ld.EPS_LD <= 2.0 ** -63


def test_newton_inverse_reaches_extended_precision():
    rng = np.random.default_rng(4)
    D = rng.standard_normal((50, 5, 5)) * np.logspace(0, 12, 5)[None, :, None]     # rows of very different size: cond up to 1e13
    X = ld.newton_inverse(D)
    res = np.abs(np.eye(5, dtype=ld.LD) - D.astype(ld.LD) @ X).max()
    assert res <= 64 * ld.EPS_LD * np.linalg.cond(D).max() and res <= 1e-4


def test_op_is_the_matrix(oracle):
    s, A, b, H, C = _system(oracle, "pihna_hub")       # one row of 740 blocks
    x = np.random.default_rng(1).standard_normal(b.size)
    op = ld.Op.of_matrix(A)
    assert np.abs(op @ x - A @ x).max() <= 1e-12 * np.abs(A @ x).max()
    lv = H[0].levels[1]
    y, A1 = x[:lv["n"] * s.nv], lv["A"]
    assert np.all(np.abs(ld.Op.of_blocks(lv["bptr"], lv["bcol"], lv["blocks"]) @ y - A1 @ y) <= 1e-12 * (abs(A1) @ np.abs(y)))
    dofs = np.array([7, 3, 11])
    assert np.array_equal((op.rows(dofs) @ x).astype(np.float64), (op @ x)[dofs].astype(np.float64))


@pytest.mark.parametrize("smoother", [0, 1])
@pytest.mark.parametrize("name", SYSTEMS)
def test_noise(oracle, name, smoother):
    """(a): the FP64 rounding of the numpy cycle, measured against the extended-precision one"""
    s, A, b, H, C = _system(oracle, name)
    n2, ninf = ld.noise(H[smoother], C[smoother], ld.probe_vectors(b.size, b))
    print(f"noise {name} {SMOOTHERS[smoother]}: 2-norm {n2:.1e}, max-norm {ninf:.1e}; levels {H[0].level_sizes()}")
    assert n2 <= 1e-9 and ninf <= 1e-9
    assert ld.bound(max(ld.MARGIN, ld.MARGIN_MIXED), n2, ninf) <= ld.BOUND_CAP


@pytest.mark.parametrize("name", SYSTEMS)
def test_mixed_noise(oracle, name):
    """(b): the mixed cycle on fl32 of numpy's D^-1 A against the mixed cycle on fl32 of the extended-precision D^-1 A, both
    evaluated in extended precision, so that only the entries of the copy that round differently tell"""
    s, A, b, H, C = _system(oracle, name)
    A32, A32x = solve_ref_mixed.scaled_f32(A, s.nv, 2), ld.scaled_f32_ld(A, s.nv)
    diff = (A32 - A32x).tocsr()
    diff.eliminate_zeros()
    at = diff.nonzero()
    ref = np.abs(np.asarray(A32x[at]).ravel())
    # an entry that is zero but for rounding (D^-1 D off the diagonal, cancellation) differs in all its digits and tells nothing;
    # a flip is an entry of ordinary size whose two roundings are neighbours in fp32
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    flips = int(np.count_nonzero((np.abs(diff.data) <= ulp) & (ref >= 2.0 ** -40 * np.abs(A32x.data).max())))
    print(f"fp32 copy of {name}: {diff.nnz} of {A32.nnz} entries differ, {flips} of them by one ulp of an entry above 2^-40 of the largest")
    for smoother in (0, 1):
        Ca, Cb = ld.Cycle(H[smoother], A, op0=A32), ld.Cycle(H[smoother], A, op0=A32x)
        d = [ld.rel_diff(Ca.cycle(v), Cb.cycle(v)) for v in ld.probe_vectors(b.size, b)]
        n32 = max(max(p) for p in d)
        print(f"noise32 {name} {SMOOTHERS[smoother]}: {n32:.1e}")
        assert n32 <= 1e-9
        # and the numpy mixed cycle is the extended one up to its own noise
        n2, ninf = ld.noise(ld.mixed_hierarchy(H[smoother], A32), Ca, ld.probe_vectors(b.size, b))
        print(f"noise (mixed form) {name} {SMOOTHERS[smoother]}: 2-norm {n2:.1e}, max-norm {ninf:.1e}")
        assert n2 <= 1e-9 and ninf <= 1e-9


# ---- (c) the faults ----

def _cycle(H, r, l=0, sweeps=COARSEST_SWEEPS, skip_last_member=(), unordered=0):
    """H.cycle of either smoother written out once more, with the places of three faults as arguments: the sweeps of the last
    level; the levels whose restriction to the next skips the last member of every aggregate; the largest level (in nodes) on
    which a Gauss-Seidel sweep ignores the colour order (every colour reads the x from before the sweep: no barrier)"""
    kw = dict(sweeps=sweeps, skip_last_member=skip_last_member, unordered=unordered)
    gs = hasattr(H, "_gs")

    def sweep(x):
        if not gs:
            return x + H._smooth(l, r - H._op(l, x))
        if H.levels[l]["n"] > unordered:
            return H._gs(l, r, x)
        x0 = x.copy()
        for dofs, rows, dinv in H.levels[l]["sweep"]:
            x[dofs] += (r[dofs] - dinv @ (rows @ x0)) if l == 0 else dinv @ (r[dofs] - rows @ x0)
        return x

    x = H._smooth(l, r)
    if l == len(H.levels) - 1:
        for _ in range(sweeps - 1):
            x = sweep(x)
        return x
    P, res = H.levels[l]["P"], r - H._op(l, x)
    if l in skip_last_member:
        agg = H.levels[l]["agg"]
        last = np.zeros(H.levels[l + 1]["n"], dtype=np.int64)
        np.maximum.at(last, agg, np.arange(agg.size))
        res = res.copy()
        res.reshape(-1, H.nv)[last] = 0.0
    x = x + P @ _cycle(H, P.T @ res, l + 1, **kw)
    return sweep(x)


def _short_galerkin(H, level=2):
    """H with every Galerkin sum of `level` that has more than one summand short of its last; the levels below follow from it"""
    G = copy.copy(H)
    G.levels = [dict(lv) for lv in H.levels]
    for l in range(level, len(G.levels)):
        lv, cptr, cidx = G.levels[l], *ld.galerkin_lists(H, l)
        if l == level:
            keep = np.ones(cidx.size, dtype=bool)
            keep[(cptr[1:] - 1)[np.diff(cptr) > 1]] = False
            cptr, cidx = np.concatenate([[0], np.cumsum(np.add.reduceat(keep, cptr[:-1]))]), cidx[keep]
        lv["blocks"] = solve_ref_mg.galerkin(G.levels[l - 1]["blocks"], cptr, cidx)
        N = lv["n"] * G.nv
        lv["A"] = sps.bsr_matrix((lv["blocks"], lv["bcol"], lv["bptr"]), shape=(N, N)).tocsr()
        lv["Dinv"] = solve_ref.precond_inverse(lv["A"], G.nv, 2)[0]
    if hasattr(G, "_gs"):
        G.colour()
    return G.cycle


MUTANTS = {   # name -> (cycle of the faulty hierarchy from the sound one, [(system, smoother)]: the rows of the record)
    "galerkin2_short": (lambda H: _short_galerkin(H), [("pihna_kuhn", 0), ("pihna_kuhn", 1), ("pihna_hydrogel", 0), ("pihna_hydrogel", 1)]),
    "coarsest_7_sweeps": (lambda H: lambda r: _cycle(H, r, sweeps=COARSEST_SWEEPS - 1), [("pihna_kuhn", 0), ("pihna_hydrogel", 0)]),
    "restrict_1_skips_last": (lambda H: lambda r: _cycle(H, r, skip_last_member=(1,)), [("pihna_kuhn", 0), ("hcc_hex", 1), ("pihna_hydrogel", 1)]),
    "gs_fused_unordered": (lambda H: lambda r: _cycle(H, r, unordered=512), [("pihna_kuhn", 1), ("hcc_hex", 1), ("pihna_hydrogel", 1)]),
}
_ROWS = {}


def _iterations(A, b, nv, cycle):
    out = []
    for rel_tol in (1e-8, 1e-10):
        _, info = solve_ref.bicgstab(A, b, np.zeros(b.size), rel_tol, 0.0, 2000, 2, nv, right=cycle)
        assert info["reason"] == solve_ref.CONVERGED
        out.append(info["iterations"])
    return out


@pytest.mark.parametrize("smoother", [0, 1])
@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex"])
def test_the_cycle_written_out_is_the_cycle(oracle, name, smoother):
    s, A, b, H, C = _system(oracle, name)
    v = np.random.default_rng(11).standard_normal(b.size)
    assert _cycle(H[smoother], v).tobytes() == H[smoother].cycle(v).tobytes()


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_faulty_cycle_moves_far_more_than_the_bound(oracle, mutant):
    make, rows = MUTANTS[mutant]
    seen = 0.0
    for name, smoother in rows:
        s, A, b, H, C = _system(oracle, name)
        h = H[smoother]
        v = ld.probe_vectors(b.size, b)[0]
        faulty = make(h)
        moved = ld.rel_diff(faulty(v), np.asarray(h.cycle(v), dtype=ld.LD))[0]
        limit = ld.bound(ld.MARGIN, *ld.noise(h, C[smoother], ld.probe_vectors(b.size, b)))
        key = (name, smoother)
        if key not in _ROWS:
            _ROWS[key] = _iterations(A, b, s.nv, h.cycle)
        its, base = _iterations(A, b, s.nv, faulty), _ROWS[key]
        kept = all(i <= y + 2 for i, y in zip(its, base))
        print(f"mutant {mutant} | {name} | {SMOOTHERS[smoother]} | iterations {its[0]} / {its[1]} ({base[0]} / {base[1]}) | "
              f"cycle moves by {moved:.1e} = {moved / limit:.1e} x bound {limit:.1e} | {'passes' if kept else 'fails'} yardstick + 2")
        _ROWS[(mutant,) + key] = (moved / limit, kept)
        seen = max(seen, moved / limit)
    assert seen >= 1000.0


def test_three_faults_pass_the_iteration_counts(oracle):
    """... on a case where the cycle moves by 1000 x the bound: what the GPU test of one cycle sees and a converged solve does not"""
    hidden = set()
    for mutant, (make, rows) in MUTANTS.items():
        for key in rows:
            if (mutant,) + key not in _ROWS:
                test_a_faulty_cycle_moves_far_more_than_the_bound(oracle, mutant)
            ratio, kept = _ROWS[(mutant,) + key]
            if kept and ratio >= 1000.0:
                hidden.add(mutant)
    print("faults that pass iterations <= yardstick + 2 on both tolerances:", sorted(hidden))
    assert len(hidden) >= 3
