"""CPU build of the multigrid-across-ranks host code of rdcfes_amd/csrc/rdc_solve.h (tests/host_solve_mg_dist_shim.cpp) against the
numpy yardstick (tests/solve_ref_mg_dist.py): every rank is fed its local pattern and the aggregate numbers the numpy exchange
delivers, and must reproduce the yardstick's aggregates, coarse patterns, gather lists, send lists, slot lists and peer offsets
on every level."""
import ctypes as C
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import solve_ref_dist
import solve_ref_mg
import solve_ref_mg_dist

ROOT = Path(__file__).resolve().parent.parent
STEP = {"agg": (0, np.int32), "mptr": (1, np.int64), "member": (2, np.int32), "bptr": (3, np.int64), "bcol": (4, np.int32),
        "cptr": (5, np.int64), "cidx": (6, np.int32), "cnode": (7, np.int32)}
HALO = {"send_off": (10, np.int64), "ghost_off": (11, np.int64), "send_nodes": (12, np.int32), "send_ptr": (13, np.int64),
        "send_slot": (14, np.int32)}


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libhost_solve_mg_dist_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_mg_dist_shim.cpp"
    hdr = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        str(src), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_dist_plan.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.shim_dist_aggregate.restype = C.c_int64
    lib.shim_dist_aggregate.argtypes = [C.c_int, C.c_void_p]
    lib.shim_dist_coarsen.argtypes = [C.c_int, C.c_void_p]
    lib.shim_dist_goes_on.argtypes = [C.c_int, C.c_double, C.c_double]
    lib.shim_dist_list.restype = C.c_int64
    lib.shim_dist_list.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.shim_dist_bytes.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return lib


def _list(lib, r, level, which, dt):
    a = np.empty(lib.shim_dist_list(r, level, which, None), dtype=dt)
    assert lib.shim_dist_list(r, level, which, a.ctypes.data) == a.size
    return a


def _plan(lib, r, lp, bptr, bcol, send_count=None, ghost_count=None):
    h = solve_ref_mg_dist.halo0(lp)
    sc = np.ascontiguousarray(np.diff(h["send_off"]) if send_count is None else send_count, dtype=np.int64)
    gc = np.ascontiguousarray(np.diff(h["ghost_off"]) if ghost_count is None else ghost_count, dtype=np.int64)
    bptr, bcol = np.ascontiguousarray(bptr, dtype=np.int64), np.ascontiguousarray(bcol, dtype=np.int32)
    send = np.ascontiguousarray(h["send_nodes"], dtype=np.int32)
    return lib.shim_dist_plan(r, h["n"], h["n_ghost"], bptr.ctypes.data, bcol.ctypes.data, send.size, send.ctypes.data, sc.size, sc.ctypes.data, gc.ctypes.data)


def _build(lib, patterns, lps):
    """drives the compiled steps rank by rank with the numpy exchange; returns the number of levels"""
    world = len(lps)
    lib.shim_dist_world(world)
    for r in range(world):
        assert _plan(lib, r, lps[r], *patterns[r]) == 0
    halos = [solve_ref_mg_dist.halo0(lp) for lp in lps]
    levels = 1
    while True:
        sends, nas = [], []
        for r in range(world):
            out = np.full(halos[r]["send_nodes"].size + 1, -7.0)
            nas.append(lib.shim_dist_aggregate(r, out.ctypes.data))
            assert out[-1] == -7.0
            sends.append(out[:-1])
        nodes, merged = sum(h["n"] for h in halos), sum(int(na < h["n"]) for na, h in zip(nas, halos))
        if not lib.shim_dist_goes_on(levels, float(nodes), float(merged)):
            return levels
        recvs = solve_ref_mg_dist.exchange_ids(halos, sends)
        for r in range(world):
            ids = np.ascontiguousarray(np.concatenate([recvs[r], [-1.0]]))
            assert lib.shim_dist_coarsen(r, ids.ctypes.data) == 1
            h = dict(peers=halos[r]["peers"], n=lib.shim_dist_list(r, levels, 110, None), n_ghost=lib.shim_dist_list(r, levels, 111, None))
            h.update({k: _list(lib, r, levels, w, dt) for k, (w, dt) in HALO.items()})
            halos[r] = h
        levels += 1


def _compare(lib, patterns, lps, nv):
    steps, halos, _ = solve_ref_mg_dist.pattern_hierarchy_dist(patterns, lps)
    levels = _build(lib, patterns, lps)
    world = len(lps)
    assert levels == len(halos[0]) and all(lib.shim_dist_list(r, 0, 120, None) == levels for r in range(world))
    for r in range(world):
        fb = np.asarray(patterns[r][0], dtype=np.int64)
        for l in range(levels):
            H = halos[r][l]
            assert (lib.shim_dist_list(r, l, 110, None), lib.shim_dist_list(r, l, 111, None)) == (H["n"], H["n_ghost"])
            for key, (which, dt) in HALO.items():
                np.testing.assert_array_equal(_list(lib, r, l, which, dt), H[key], err_msg=f"rank {r} level {l} {key}")
        for l, st in enumerate(steps[r]):
            n_fine = halos[r][l]["n"]
            assert (lib.shim_dist_list(r, l, 100, None), lib.shim_dist_list(r, l, 101, None), lib.shim_dist_list(r, l, 102, None)) == \
                (n_fine, st["n"], st["n_pass1"])
            got = {k: _list(lib, r, l, w, dt) for k, (w, dt) in STEP.items()}
            for key in ("agg", "bptr", "bcol", "cptr", "cidx"):
                np.testing.assert_array_equal(got[key], st[key], err_msg=f"rank {r} step {l} {key}")
            # members: the inverse of the owned part of agg, ascending; contributions name their row node
            np.testing.assert_array_equal(np.diff(got["mptr"]), np.bincount(st["agg"][:n_fine], minlength=st["n"]))
            np.testing.assert_array_equal(got["member"], np.argsort(st["agg"][:n_fine], kind="stable"))
            np.testing.assert_array_equal(got["cnode"], np.repeat(np.arange(n_fine), np.diff(fb))[got["cidx"]])
            fb = st["bptr"]
        out = (C.c_int64 * 2)()
        assert lib.shim_dist_bytes(r, nv, out) == levels and out[1] > 0 and out[0] % 256 == 0 and out[1] % 256 == 0
    return steps, halos


@pytest.mark.parametrize("name,world", [("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("hcc_hex", 3), ("pihna_kuhn3", 3)])
def test_hierarchy_of_every_rank_against_numpy(oracle, lib, name, world):
    s = solve_ref_dist.case(name)
    ranks = solve_ref_dist.ranks_of(name, world, oracle)
    patterns = [solve_ref_mg.block_pattern(rk.A, s.nv)[:2] for rk in ranks]
    steps, halos = _compare(lib, patterns, [rk.lp for rk in ranks], s.nv)
    print(name, world, "levels per rank (owned + ghost):", [[(h["n"], h["n_ghost"]) for h in hr] for hr in halos])
    # for every pair and level: r's send segment for q and q's ghost segment from r name the same aggregates in the same order
    for l in range(1, len(halos[0])):
        for r in range(world):
            for k, q in enumerate(halos[r][l]["peers"]):
                j = halos[q][l]["peers"].index(r)
                seg = _list(lib, r, l, 12, np.int32)[halos[r][l]["send_off"][k]:halos[r][l]["send_off"][k + 1]]
                # q's ghosts from r, as q numbers them, are consecutive from q's n + ghost_off[j]: the i-th is r's aggregate seg[i]
                fine_q = halos[q][l - 1]
                agg_q = _list(lib, q, l - 1, 0, np.int32)
                tail = agg_q[fine_q["n"] + fine_q["ghost_off"][j]:fine_q["n"] + fine_q["ghost_off"][j + 1]] - halos[q][l]["n"] - halos[q][l]["ghost_off"][j]
                agg_r = _list(lib, r, l - 1, 0, np.int32)
                fine_r = halos[r][l - 1]
                sent = agg_r[fine_r["send_nodes"][fine_r["send_off"][k]:fine_r["send_off"][k + 1]]]
                np.testing.assert_array_equal(seg[tail], sent)
                assert seg.size == halos[q][l]["ghost_off"][j + 1] - halos[q][l]["ghost_off"][j] and np.unique(seg).size == seg.size


def _unconnected_world():
    """two ranks: rank 0 owns a 5 x 10 grid graph, rank 1 owns 10 nodes that are mutually unconnected, node i of it coupled to node
    i of rank 0 only.  Rank 1 can merge nothing while rank 0 does."""
    adj = [set([i]) for i in range(50)]
    for i in range(5):
        for j in range(10):
            a = i * 10 + j
            if j + 1 < 10:
                adj[a].add(a + 1), adj[a + 1].add(a)
            if i + 1 < 5:
                adj[a].add(a + 10), adj[a + 10].add(a)
    for i in range(10):
        adj[i].add(50 + i)                   # rank 1's node i is rank 0's ghost 50 + i
    rows0 = [sorted(a) for a in adj]
    rows1 = [[i, 10 + i] for i in range(10)]    # itself and rank 0's node i, its ghost 10 + i
    pat = lambda rows: (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int32))
    lp0 = SimpleNamespace(rank=0, n_owned=50, xyz=np.zeros((60, 3)), send_ids={1: np.arange(10)}, recv_ids={1: np.arange(50, 60)})
    lp1 = SimpleNamespace(rank=1, n_owned=10, xyz=np.zeros((20, 3)), send_ids={0: np.arange(10)}, recv_ids={0: np.arange(10, 20)})
    return [pat(rows0), pat(rows1)], [lp0, lp1]


def test_a_rank_that_merges_nothing_goes_on_with_the_identity(lib):
    patterns, lps = _unconnected_world()
    steps, halos = _compare(lib, patterns, lps, 3)
    assert len(steps[0]) >= 1
    np.testing.assert_array_equal(steps[1][0]["agg"][:10], np.arange(10))       # identity on rank 1 ...
    assert steps[0][0]["n"] < 50 and steps[1][0]["n"] == 10                      # ... while rank 0 merged
    assert halos[1][1]["n_ghost"] <= 10 and halos[0][1]["n_ghost"] == 10       # rank 0 sees all ten of rank 1's singletons


def test_plan_peers_argument_checks(lib):
    patterns, lps = _unconnected_world()
    lib.shim_dist_world(2)
    assert _plan(lib, 0, lps[0], *patterns[0]) == 0
    assert _plan(lib, 0, lps[0], *patterns[0], send_count=[-1]) == 1
    assert _plan(lib, 0, lps[0], *patterns[0], send_count=[9]) == 2
    assert _plan(lib, 0, lps[0], *patterns[0], ghost_count=[11]) == 3
    assert _plan(lib, 0, lps[0], *patterns[0], send_count=[4, 6], ghost_count=[10, 0]) == 0      # zeros and more peers are allowed
    bad = SimpleNamespace(rank=0, n_owned=50, xyz=np.zeros((60, 3)), send_ids={1: np.arange(45, 55)}, recv_ids={1: np.arange(50, 60)})
    assert _plan(lib, 0, bad, *patterns[0]) == 4
