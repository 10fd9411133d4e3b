"""CPU build of what rdc_solid_newton_dist decides on the host (rdcfes_amd/csrc/rdc_newton.h, compiled by g++ into
tests/host_newton_dist_main.cpp): which partitioned linear entry every (precond, "solve_method") goes to, which callbacks of
rdc_solve_comm_wide that entry needs, and the layout of the work memory with the ghost tail behind delta (newton_carve_dist), with
what newton_carve returns left as it was.  The same program is built once more under AddressSanitizer + UBSan and must run clean."""
import itertools
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_newton_dist_main.cpp"
DEPS = [SRC, ROOT / "rdcfes_amd" / "csrc" / "rdc_newton.h", ROOT / "include" / "rdc_assembly.h"]
DIST, DIST_MG, DIST_GMRES = 0, 1, 2
NEEDS_SIZED, NEEDS_WIDE = 1, 2
BEGIN, END, SUM, SIZED_BEGIN, SIZED_END, WIDE = (1 << k for k in range(6))
CHUNK, ALIGN, REC = 1024, 32, 8
# (n_node, n_owned, n_send): the cube on three ranks (ISSUE: 300/239/190 owned, 91/116/99 ghosts), no ghosts, a rank that owns
# nothing, nothing at all, sizes next to the alignment and the chunk, and past 2^31 entries
SHAPES = [(391, 300, 95), (355, 239, 140), (289, 190, 104), (729, 729, 0), (40, 0, 0), (0, 0, 0), (11, 10, 11), (342, 341, 1),
          (1025, 1024, 3), (1 << 30, (1 << 30) - 5, 1 << 20)]


def _build(out, flags):
    out.parent.mkdir(exist_ok=True)
    if not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in DEPS):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, str(SRC), "-o", str(out)], check=True)
    return out


def _runner(out):
    def run(text):
        r = subprocess.run([str(out)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stderr == "", r.stderr
        return [ln.split() for ln in r.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def prog():
    return _runner(_build(ROOT / "tests" / "_build" / "host_newton_dist_main", ["-O2", "-ffp-contract=off"]))


def want_dispatch(precond, method):
    """the table of the issue: "solve_method" = 1 -> gmres; otherwise precond 3 or 6 -> mg; otherwise dist"""
    mg = precond in (3, 6)
    entry = DIST_GMRES if method == 1 else DIST_MG if mg else DIST
    return entry, (NEEDS_SIZED if mg else 0) | (NEEDS_WIDE if method == 1 else 0)


def test_dispatch_table(prog):
    cases = list(itertools.product(range(7), (0, 1)))
    got = prog("".join(f"dispatch {p} {m}\n" for p, m in cases))
    assert len(got) == len(cases)
    for (p, m), line in zip(cases, got):
        assert line[0] == "dispatch" and (int(line[1]), int(line[2])) == want_dispatch(p, m), (p, m, line)
    # spelled out once, so that the restatement above cannot be wrong in the same way
    table = {(p, m): (int(l[1]), int(l[2])) for (p, m), l in zip(cases, got)}
    assert table[(2, 0)] == (DIST, 0) and table[(5, 0)] == (DIST, 0) and table[(4, 0)] == (DIST, 0) and table[(0, 0)] == (DIST, 0)
    assert table[(3, 0)] == (DIST_MG, NEEDS_SIZED) and table[(6, 0)] == (DIST_MG, NEEDS_SIZED)
    assert table[(2, 1)] == (DIST_GMRES, NEEDS_WIDE) and table[(5, 1)] == (DIST_GMRES, NEEDS_WIDE)
    assert table[(3, 1)] == (DIST_GMRES, NEEDS_SIZED | NEEDS_WIDE) and table[(6, 1)] == (DIST_GMRES, NEEDS_SIZED | NEEDS_WIDE)


def test_required_callbacks(prog):
    """for every (precond, method) and every subset of the six callbacks: complete exactly when the three of the base are there,
    the sized pair if the entry runs the multigrid, the wide all-reduce if it is GMRES"""
    cases = list(itertools.product(range(7), (0, 1), range(64)))
    got = prog("".join(f"complete {p} {m} {mask}\n" for p, m, mask in cases))
    assert len(got) == len(cases)
    for (p, m, mask), line in zip(cases, got):
        need = BEGIN | END | SUM
        if p in (3, 6):
            need |= SIZED_BEGIN | SIZED_END
        if m == 1:
            need |= WIDE
        assert int(line[1]) == int(mask & need == need), (p, m, mask, line)


def _up(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def _fields(line):
    keys = ("n", "n_owned", "blocks", "u0", "delta", "partials", "rec", "bytes", "n_delta", "send", "n_send")
    return dict(zip(keys, map(int, line[1:])))


def test_carve_dist_layout(prog):
    got = prog("".join(f"carve_dist {a} {b} {c}\n" for a, b, c in SHAPES))
    for (n_node, n_owned, n_send), line in zip(SHAPES, got):
        w = _fields(line)
        assert (w["n"], w["n_owned"], w["n_delta"], w["n_send"]) == (3 * n_node, 3 * n_owned, 3 * n_node, 3 * n_send)
        assert w["blocks"] == (3 * n_node + CHUNK - 1) // CHUNK
        parts = [(w["u0"], w["n"]), (w["delta"], w["n_delta"]), (w["partials"], 2 * w["blocks"]), (w["send"], w["n_send"]), (w["rec"], REC)]
        at = 0
        for off, size in parts:             # in this order, each on a 256-byte boundary, none reaching into the next
            assert off % ALIGN == 0 and off >= at, (n_node, n_owned, n_send, parts)
            at = off + size
        assert w["bytes"] == 8 * at and w["bytes"] % 64 == 0      # the record is the last part: 64 bytes
        assert w["delta"] - w["u0"] >= w["n"] and w["partials"] - w["delta"] >= w["n_delta"]   # delta has its ghost tail


def test_old_carve_is_unchanged(prog):
    """newton_carve as tests/test_host_newton.py states it, and equal to newton_carve_dist where there is no ghost and no send list"""
    got = prog("".join(f"carve {a} {b}\ncarve_dist {a} {b} 0\n" for a, b, _ in SHAPES))
    for k, (n_node, n_owned, _) in enumerate(SHAPES):
        w, wd = _fields(got[2 * k]), _fields(got[2 * k + 1])
        n, no = 3 * n_node, 3 * n_owned
        blocks = (n + CHUNK - 1) // CHUNK
        u0, delta = 0, _up(n)
        partials = delta + _up(no)
        rec = partials + _up(2 * blocks)
        assert (w["n"], w["n_owned"], w["blocks"], w["u0"], w["delta"], w["partials"], w["rec"]) == (n, no, blocks, u0, delta, partials, rec)
        assert w["bytes"] == 8 * (rec + REC) and w["n_delta"] == no and w["n_send"] == 0 and w["send"] == rec
        if n_node == n_owned:
            assert w == dict(wd, n_delta=no)
            assert wd["n_delta"] == n == no


def test_stand_alone_program_under_sanitizers():
    run = _runner(_build(ROOT / "tests" / "_build" / "host_newton_dist_asan",
                         ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]))
    text = "".join(f"dispatch {p} {m}\n" for p in range(-1, 9) for m in (-1, 0, 1, 2))
    text += "".join(f"complete {p} {m} {mask}\n" for p in range(7) for m in (0, 1) for mask in range(64))
    text += "".join(f"carve {a} {b}\ncarve_dist {a} {b} {c}\n" for a, b, c in SHAPES)
    out = run(text)
    assert len(out) == 40 + 7 * 2 * 64 + 2 * len(SHAPES)
