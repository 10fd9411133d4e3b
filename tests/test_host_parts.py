"""Two-part assembly on the CPU: the splits of rdcfes_amd/csrc/rdc_parts.h (which work items of a family of lists are interior
for a given "interior_nodes", and which rows are complete once they have run) through the host shim, each against a brute-force
statement of the same thing."""
import ctypes as C

import numpy as np
import pytest

from rdcfes_amd import partition, synth

EV_DESC = np.dtype([("nown", "<u4"), ("nvis", "<u4"), ("ntouch", "<u4"), ("nb", "<u4"), ("out_doubles", "<u4"),
                    ("min_node", "<u4"), ("max_node", "<u4"), ("pad", "<u4")])


def _mesh(name):
    """(conn, n_node, n_owned)"""
    if name == "ghosted":      # one rank of K(8) split in three: its owned nodes come first, ghosts behind them
        conn, xyz = synth.kuhn_tet_mesh(8, order="random")
        lp = partition.build_local(conn, xyz, partition.partition_rcb(xyz[conn].mean(axis=1), 3), 1, 3)
        assert lp.n_owned < lp.xyz.shape[0]
        return lp.conn, lp.xyz.shape[0], lp.n_owned
    conn, xyz = synth.kuhn_tet_mesh(6, order=name)
    return conn, xyz.shape[0], xyz.shape[0]


# "interior_nodes" as a function of n_owned, and whether the element-visit lists are built with it (None: as the context does,
# which passes it on when it does not exceed n_owned) or without it (a context whose option was set after the upload)
CASES = {"none": (lambda n: 0, None), "some": (lambda n: int(0.37 * n), None), "all": (lambda n: n, None),
         "beyond": (lambda n: n + 5, None), "set_after_upload": (lambda n: int(0.37 * n), -1)}


@pytest.fixture(scope="module", params=["lex", "random", "ghosted"])
def mesh(request):
    return _mesh(request.param)


@pytest.fixture
def lists(mesh, make_prep):
    """the pair lists (numpy view) of the mesh, which is then the shim's current one (the element-visit lists are built on it)"""
    conn, n_node, n_owned = mesh
    P = make_prep(4, conn, n_node, n_owned, 5)
    assert P.ok and P.rg2_ok, P.error
    return P, n_owned


def _ev_lists(shim, n_interior):
    """(descriptors, owned nodes per cluster) of the element-visit lists built on the last prep"""
    st = (C.c_int64 * 6)()
    shim.shim_ev_build_interior.argtypes = [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    assert shim.shim_ev_build_interior(54000, n_interior, st) == 0, shim.shim_prep_error()
    desc = np.empty(shim.shim_prep_size(31) // EV_DESC.itemsize, dtype=EV_DESC)
    shim.shim_prep_copy(31, desc.ctypes.data_as(C.c_void_p))
    nlist = np.empty(shim.shim_prep_size(35), dtype=np.uint32)
    shim.shim_prep_copy(35, nlist.ctypes.data_as(C.c_void_p))
    nlist = nlist.reshape(desc.size, st[3])
    owned = [nlist[w, :desc["nown"][w]].astype(np.int64) for w in range(desc.size)]     # the owned nodes lead a cluster's list
    return desc, owned


@pytest.mark.parametrize("case", list(CASES))
def test_split_of_the_element_visit_lists(shim, lists, case):
    P, n_owned = lists
    interior = CASES[case][0](n_owned)
    built_with = CASES[case][1] if CASES[case][1] is not None else (interior if interior <= n_owned else -1)
    desc, owned = _ev_lists(shim, built_with)
    n_wg = desc.size
    assert sorted(np.concatenate(owned).tolist()) == list(range(n_owned))
    assert all(o.min() == desc["min_node"][w] and o.max() == desc["max_node"][w] for w, o in enumerate(owned))
    out = (C.c_int64 * 2)()
    perm = np.full(n_wg + 8, 0xFFFFFFFF, dtype=np.uint32)
    shim.shim_split_ev.restype = C.c_int64
    shim.shim_split_ev.argtypes = [C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int64]
    assert shim.shim_split_ev(interior, out, perm.ctypes.data_as(C.c_void_p), perm.size) == n_wg
    wg, nodes = list(out)
    perm = perm[:n_wg].astype(np.int64)
    assert sorted(perm.tolist()) == list(range(n_wg))                            # a permutation of all clusters
    is_interior = np.array([o.max() < interior for o in owned])
    assert wg == int(is_interior.sum())
    assert perm[:wg].tolist() == np.flatnonzero(is_interior).tolist()            # exactly the interior clusters, in list order
    assert perm[wg:].tolist() == np.flatnonzero(~is_interior).tolist()           # then the others, in list order
    behind = np.concatenate([owned[w] for w in perm[wg:]]) if wg < n_wg else np.empty(0, dtype=np.int64)
    assert not (behind < nodes).any()                                            # rows [0, nodes) are complete after part 1 ...
    assert 0 <= nodes <= interior
    assert nodes == interior or (behind < nodes + 1).any()                       # ... and nodes is the largest such bound
    mixed = int(sum((o.min() < interior <= o.max()) for o in owned))
    if CASES[case][1] is None and interior <= n_owned:
        assert mixed == 0 and nodes == interior       # lists built for this value: no cluster holds both kinds
    elif case == "set_after_upload":
        assert mixed > 0 and nodes < interior         # the case is what it claims to be
    # the permutation is an optional output: the same split without it
    out2 = (C.c_int64 * 2)()
    assert shim.shim_split_ev(interior, out2, None, 0) == 0 and list(out2) == [wg, nodes]


@pytest.mark.parametrize("case", [c for c in CASES if c != "set_after_upload"])      # the pair lists do not depend on the option
def test_split_of_the_pair_lists(shim, lists, case):
    P, n_owned = lists
    interior = CASES[case][0](n_owned)
    ends = P.wg2["n0"].astype(np.int64) + P.wg2["nnodes"]
    assert ends.size > 1 and ends[-1] == n_owned
    wg = 0
    while wg < ends.size and ends[wg] <= interior:
        wg += 1
    out = (C.c_int64 * 2)()
    shim.shim_split_pairs.argtypes = [C.c_int64, C.POINTER(C.c_int64)]
    shim.shim_split_pairs(interior, out)
    assert list(out) == [wg, int(ends[wg - 1]) if wg else 0]
    if case == "some":
        assert 0 < wg < ends.size
