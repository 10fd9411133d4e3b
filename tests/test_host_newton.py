"""CPU build of rdcfes_amd/csrc/rdc_newton.h as compiled by g++ (tests/host_newton_main.cpp): every decision of rdc_solid_newton
(newton_next) driven with scripted norms against a restatement of SolidSystem::solve() in its loop form; the layout of the work
memory (newton_carve); the refusals of the parameters; the sizes of the two C structs against their ctypes mirrors."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FULL, SOLVE, TRY, HALVE, ACCEPT, FINISH = range(6)
CONV_RES, CONV_STEP, MAX_ITS, LIN_FAILED, NOT_FINITE = range(5)
NAN = float("nan")


@pytest.fixture(scope="module")
def prog():
    out = ROOT / "tests" / "_build" / "host_newton_main"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_newton_main.cpp"
    deps = [src, ROOT / "rdcfes_amd" / "csrc" / "rdc_newton.h", ROOT / "include" / "rdc_assembly.h"]
    if not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", str(src), "-o", str(out)], check=True)

    def run(text):
        r = subprocess.run([str(out)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return [ln.split() for ln in r.stdout.splitlines()]
    return run


def restate(p, script):
    """SolidSystem::solve() of rdc_host.h as a loop over scripted measurements: script = [(residual, step_norm, solution_norm,
    linear_reason, linear_iterations)], one entry per action.  -> (actions [(action, measure, restore, step, it)], info tuple)"""
    feed = iter(script)
    acts = []
    I = dict(reason=0, nl=0, li=0, asm=0, halv=0, llr=0, first=0.0, last=0.0, dn=0.0, un=0.0)
    it, step, saved = 0, 1.0, False

    def emit(a, measure=0, restore=0):
        acts.append((a, int(measure), int(restore), step, it))

    def finish(reason, restore=False):
        I["reason"] = reason
        emit(FINISH, 0, restore)
        return acts, (I["reason"], I["nl"], I["li"], I["asm"], I["halv"], I["llr"], I["first"], I["last"], I["dn"], I["un"])

    while True:
        emit(FULL)
        rn = next(feed)[0]
        I["asm"] += 1
        if it == 0:
            I["first"] = rn
        I["last"] = rn
        if not math.isfinite(rn):
            return finish(NOT_FINITE, saved)
        if rn <= p["abs_res"] or rn <= p["rel_res"] * I["first"]:
            return finish(CONV_RES)
        if it >= p["max"]:
            return finish(MAX_ITS)
        emit(SOLVE)
        _, _, _, lreason, lits = next(feed)
        saved = True
        I["li"] += lits
        I["llr"] = lreason
        if lreason not in (0, 1):
            return finish(LIN_FAILED)
        step, act = 1.0, TRY
        while True:
            measure = p["req"] and not step < 1e-3
            emit(act, measure)
            rt, dn, un, _, _ = next(feed)
            I["dn"], I["un"] = dn, un
            if measure:
                I["asm"] += 1
            if not measure or rt < rn:
                break
            step *= 0.5
            I["halv"] += 1
            act = HALVE
        I["nl"] = it + 1
        by_step = dn <= p["rel_step"] * un
        emit(ACCEPT, by_step)
        rc = next(feed)[0]
        if by_step:
            I["asm"] += 1
            I["last"] = rc
            return finish(CONV_STEP) if math.isfinite(rc) else finish(NOT_FINITE, True)
        it += 1


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _drive(prog, p, script):
    text = f"run {p['max']} {int(p['req'])} {p['rel_step']!r} {p['rel_res']!r} {p['abs_res']!r} {len(script)}\n"
    text += "".join(" ".join(repr(float(v)) if i < 3 else str(int(v)) for i, v in enumerate(ln)) + "\n" for ln in script)
    out = prog(text)
    acts = [(int(t[1]), int(t[3]), int(t[5]), float(t[7]), int(t[9])) for t in out if t[0] == "act"]
    (info,) = [t for t in out if t[0] == "info"]
    info = tuple(int(v) for v in info[1:7]) + tuple(float(v) for v in info[7:])
    want_acts, want_info = restate(p, script)
    assert len(acts) == len(want_acts) and all(all(_same(x, y) for x, y in zip(a, w)) for a, w in zip(acts, want_acts)), (acts, want_acts)
    assert all(_same(x, float(y) if isinstance(x, float) else y) for x, y in zip(info, want_info)), (info, want_info)
    return acts, info


P0 = dict(max=10, req=False, rel_step=0.0, rel_res=1e-8, abs_res=1e-8)
L = (0.0, 0.0, 0.0, 0, 7)                     # a converged linear solve of 7 iterations


def R(r):
    return (r, 0.0, 0.0, 0, 0)


def S(rt, dn=1.0, un=10.0):
    return (rt, dn, un, 0, 0)


def test_residual_convergence_at_iteration_0(prog):
    acts, info = _drive(prog, P0, [R(5e-9)])
    assert [a[0] for a in acts] == [FULL, FINISH] and info[:4] == (CONV_RES, 0, 0, 1) and info[6] == info[7] == 5e-9


def test_residual_convergence_after_two_iterations(prog):
    acts, info = _drive(prog, P0, [R(1e3), L, S(0.0), R(0.0), R(1.0), L, S(0.0), R(0.0), R(1e-6)])
    assert [a[0] for a in acts] == [FULL, SOLVE, TRY, ACCEPT] * 2 + [FULL, FINISH]
    assert info[:6] == (CONV_RES, 2, 14, 3, 0, 0) and info[6] == 1e3 and info[7] == 1e-6


def test_step_convergence(prog):
    p = dict(P0, rel_step=1e-3)
    acts, info = _drive(prog, p, [R(1e3), L, S(0.0, 1e-3, 1.0), R(0.25)])
    assert [a[0] for a in acts] == [FULL, SOLVE, TRY, ACCEPT, FINISH] and acts[3][1] == 1     # the ACCEPT measures the closing residual
    assert info[:4] == (CONV_STEP, 1, 7, 2) and info[7] == 0.25 and info[8] == 1e-3 and info[9] == 1.0
    acts, info = _drive(prog, p, [R(1e3), L, S(0.0, 1.0001e-3, 1.0), R(0.0), R(0.0)])            # just above: goes on
    assert [a[0] for a in acts] == [FULL, SOLVE, TRY, ACCEPT, FULL, FINISH]


def test_max_iterations(prog):
    p = dict(P0, max=2)
    acts, info = _drive(prog, p, [R(1e3), L, S(0.0), R(0.0), R(9e2), L, S(0.0), R(0.0), R(8e2)])
    assert acts[-1][0] == FINISH and info[:4] == (MAX_ITS, 2, 14, 3)
    acts, info = _drive(prog, dict(P0, max=1), [R(1e3), L, S(0.0), R(0.0), R(9e2)])
    assert info[:4] == (MAX_ITS, 1, 7, 2)


def test_halving_accepts_a_reduction(prog):
    p = dict(P0, req=True)
    acts, info = _drive(prog, p, [R(100.0), L, S(500.0), S(100.0), S(99.0), R(0.0), R(1e-9)])   # equal is not a reduction
    assert [a[0] for a in acts] == [FULL, SOLVE, TRY, HALVE, HALVE, ACCEPT, FULL, FINISH]
    assert [a[3] for a in acts[2:5]] == [1.0, 0.5, 0.25] and all(a[1] == 1 for a in acts[2:5])
    assert info[:5] == (CONV_RES, 1, 7, 5, 2)


def test_halving_down_to_the_smallest_step(prog):
    p = dict(P0, req=True, max=1)
    trials = [S(1e9)] * 10 + [S(NAN)]       # ten measured trials (1 .. 2^-9), then 2^-10 < 1e-3 is taken unmeasured
    acts, info = _drive(prog, p, [R(100.0), L] + trials + [R(0.0), R(50.0)])
    kinds = [a[0] for a in acts]
    assert kinds == [FULL, SOLVE, TRY] + [HALVE] * 10 + [ACCEPT, FULL, FINISH]
    assert acts[12][3] == 2.0 ** -10 and acts[12][1] == 0 and all(a[1] == 1 for a in acts[2:12])
    assert info[:5] == (MAX_ITS, 1, 7, 12, 10)


def test_a_trial_residual_that_is_not_finite_halves(prog):
    p = dict(P0, req=True)
    acts, info = _drive(prog, p, [R(100.0), L, S(NAN), S(float("inf")), S(1.0), R(0.0), R(0.0)])
    assert [a[0] for a in acts] == [FULL, SOLVE, TRY, HALVE, HALVE, ACCEPT, FULL, FINISH] and info[0] == CONV_RES and info[4] == 2


@pytest.mark.parametrize("bad", [NAN, float("inf")])
def test_nan_residual(prog, bad):
    acts, info = _drive(prog, P0, [R(bad)])                                     # at the start: nothing was saved, nothing is restored
    assert [a[0] for a in acts] == [FULL, FINISH] and acts[-1][2] == 0 and info[:4] == (NOT_FINITE, 0, 0, 1)
    acts, info = _drive(prog, P0, [R(1e3), L, S(0.0), R(0.0), R(bad)])         # behind a step: back to the saved iterate
    assert acts[-1][0] == FINISH and acts[-1][2] == 1 and info[:4] == (NOT_FINITE, 1, 7, 2) and info[6] == 1e3
    acts, info = _drive(prog, dict(P0, rel_step=1.0), [R(1e3), L, S(0.0), R(bad)])   # the closing residual of a stop by step
    assert acts[-1][2] == 1 and info[:4] == (NOT_FINITE, 1, 7, 2)


@pytest.mark.parametrize("reason,goes_on", [(0, True), (1, True), (2, False), (3, False), (4, False)])
def test_each_linear_reason(prog, reason, goes_on):
    acts, info = _drive(prog, P0, [R(1e3), (0.0, 0.0, 0.0, reason, 5), S(0.0), R(0.0), R(0.0)])
    if goes_on:   # RDC_SOLVE_CONVERGED, and RDC_SOLVE_MAX_ITS used as it is
        assert [a[0] for a in acts] == [FULL, SOLVE, TRY, ACCEPT, FULL, FINISH] and info[:6] == (CONV_RES, 1, 5, 2, 0, reason)
    else:
        assert [a[0] for a in acts] == [FULL, SOLVE, FINISH] and acts[-1][2] == 0 and info[:6] == (LIN_FAILED, 0, 5, 1, 0, reason)


def test_the_loop_is_bounded(prog):
    """the worst case: every iteration halves ten times; 1000 iterations end by the cap"""
    p = dict(P0, req=True, max=1000)
    script = []
    for _ in range(1000):
        script += [R(100.0), L] + [S(1e9)] * 11 + [R(0.0)]
    acts, info = _drive(prog, p, script + [R(100.0)])
    assert info[:5] == (MAX_ITS, 1000, 7000, 11001, 10000) and len(acts) == 14 * 1000 + 2


@pytest.mark.parametrize("n_node,n_owned", [(1, 1), (729, 729), (1569, 1569), (341, 341), (342, 342), (2 ** 21 + 3, 2 ** 21 + 3), (2 ** 30, 2 ** 30)])
def test_layout(prog, n_node, n_owned):
    (c,) = [t for t in prog("constants\n") if t[0] == "constants"]
    chunk, align, rec_doubles, rec_bytes = map(int, c[1:])
    assert rec_bytes == 8 * rec_doubles == 64 and chunk == 1024 and align * 8 == 256
    (t,) = prog(f"carve {n_node} {n_owned}\n")
    n, no, blocks, u0, delta, partials, rec, nbytes = map(int, t[1:])
    assert n == 3 * n_node and no == 3 * n_owned and blocks == -(-n // chunk)
    size = dict(u0=n, delta=no, partials=2 * blocks, rec=rec_doubles)
    off = dict(u0=u0, delta=delta, partials=partials, rec=rec)
    at = 0
    for name in sorted(off, key=off.get):          # in address order: aligned, no overlap, no gap beyond the alignment
        assert off[name] % align == 0 and at <= off[name] < at + align, (name, off)
        at = off[name] + size[name]
    assert nbytes == 8 * at


def test_parameter_refusals(prog):
    ok = dict(max=10, req=0, rel_step=1e-3, rel_res=1e-8, abs_res=1e-8, lrel=1e-3, labs=0.0, lmax=50000, precond=2, mixed=0)

    def check(**kw):
        d = dict(ok, **kw)
        (t,) = prog("check " + " ".join(str(d[k]) for k in ok) + "\n")
        return int(t[1])
    assert check() == 1 and check(max=1) == 1 and check(max=1000) == 1 and check(rel_step=0.0) == 1
    assert all(check(precond=k) == 1 for k in range(7)) and check(mixed=1, req=1) == 1
    assert check(max=0) == 0 and check(max=1001) == 0 and check(max=-3) == 0
    for key in ("rel_step", "rel_res", "abs_res", "lrel", "labs"):
        assert check(**{key: "nan"}) == 0 and check(**{key: -1e-3}) == 0 and check(**{key: "inf"}) == 0, key
    assert check(precond=7) == 0 and check(precond=-1) == 0 and check(lmax=0) == 0 and check(mixed=2) == 0 and check(req=-1) == 0


def test_struct_sizes_match_the_ctypes_mirrors(prog):
    from rdcfes_amd.params import SolidNewtonInfo, SolidNewtonParams
    (t,) = prog("sizes\n")
    assert (int(t[1]), int(t[2])) == (C.sizeof(SolidNewtonParams), C.sizeof(SolidNewtonInfo)) == (72, 64)
