"""The a rows (cytokine equation, row 4 of every node) of the PIHNA element-visit kernels (rdcfes_amd/csrc/rdc_const_rows.h): with
uptake/a/from/v = 0 they do not depend on the unknowns, and a launch that finds them in memory from an earlier one writes four of
the five equation rows (k_tet4_ev / k_tet4_evq with NROW = 4: 20 len instead of 25 len doubles per segment).

Meshes: the four of test_gpu_ev_copyout.py -- K(3), K(4), K(6) in random order and hub15: rows of 5, 7, 8, 9, 11, 15 and 16 node
blocks, both 16-byte phases (asserted below: 20 len is even, so the odd tail of a shortened segment occurs exactly when the phase is
1), clusters of at most 8 owned nodes and of 9-16 (both image halves), segments shorter than one wave instruction.

States: A = synth.pihna_fields (background and a tumour sphere); B, C, ... = the tumour state at every node, each from its own seed
("dense": no noise blocks, see test_gpu_ev_copyout.py).  Every comparison is against the oracle's assembly of the state, parameters
and coordinates of THAT call, TOL = 1e-10 per block (parity.assert_csr_close), the a rows included.

"const_rows" = 2 lets a test observe the skip: a sentinel written through rdc_csr_values_device_ptr survives in the a rows exactly
when the launch left them."""
import numpy as np
import pytest

from parity import assert_csr_close
from rdcfes_amd import AssemblyContext, partition, pihna_params_from_dict, synth
from rdcfes_amd.context import FIELD_OLD_SOLUTION
from test_gpu_ev_copyout import EVQ_OPTS, _mesh

pytestmark = pytest.mark.gpu
TOL = 1e-10          # test_gpu_parity.TOL
SENTINEL = -7.25e33
MESHES = ["k3", "k4", "k6", "hub15"]
_REF = {}


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _params(pv="shipped", **changes):
    d = synth.pihna_param_dict(pv)
    assert all(k in d for k in changes)
    d.update(changes)
    return pihna_params_from_dict(d)


def _state(xyz, seed):
    """seed 0: state A; otherwise a dense state of its own"""
    return synth.pihna_fields(xyz) if seed == 0 else synth.pihna_fields(xyz, seed=synth.SEED + 10 * seed, radius=2.0)


def _oracle(oracle, name, pv, changes, seed, moved=False):
    """the oracle's system of (mesh, parameters, state, coordinates): computed once, never modified"""
    key = (name, pv, tuple(sorted(changes.items())), seed, moved)
    if key not in _REF:
        conn, xyz = _mesh(name)
        x = _moved(xyz) if moved else xyz
        ref = oracle.assemble(0, 4, conn, x, 5, _params(pv, **changes), u_old=_state(xyz, seed))
        for a in ref:
            a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _moved(xyz):
    return np.ascontiguousarray(xyz * np.array([1.1, 0.9, 1.05]) + 0.01)   # affine: every element keeps its orientation


def _a_rows(rp):
    """mask over the CSR values: the entries of the a equation's rows"""
    return np.repeat(np.arange(rp.size - 1) % 5 == 4, np.diff(rp))


def _values_tensor(ctx, nnz):
    """zero-copy torch view of the context's value array (rdc_csr_values_device_ptr)"""
    import torch

    class _View:
        pass
    v = _View()
    v.__cuda_array_interface__ = {"shape": (nnz,), "typestr": "<f8", "data": (ctx.csr_values_device_ptr()[0], False), "version": 2, "strides": None}
    return torch.as_tensor(v, device=torch.device("cuda", 0))


def _expect(ctx, ref, what):
    """the context's system equals the oracle's, every a row included, and holds no sentinel"""
    rp0, col0, val0, rhs0 = ref
    val, rhs = ctx.csr_download()
    e_val, e_rhs = rel(val, val0), rel(rhs, rhs0)
    print(f"{what}: rel(val) {e_val:.3e} rel(rhs) {e_rhs:.3e} sentinels {int((val == SENTINEL).sum())}")
    assert not (val == SENTINEL).any(), what
    assert e_val < TOL and e_rhs < TOL, what
    assert_csr_close(rp0, col0, val, val0, rhs, rhs0, 5)


def test_both_phases_and_odd_tails_of_the_shortened_segments(shim, make_prep):
    """what the cases below rely on: segments of 20 len doubles start at both 16-byte phases on every mesh (phase 1: odd head AND odd
    tail; phase 0: neither), and the row lengths are those of test_gpu_ev_copyout.py"""
    lens = set()
    for name in MESHES:
        conn, xyz = _mesh(name)
        P = make_prep(4, conn, xyz.shape[0], xyz.shape[0], 5)
        assert P.ok and P.rg2_ok, P.error
        ln = np.diff(P.bptr)
        phase = (25 * P.bptr[:-1]) & 1                                # evl::seg_phase of a node's segment in memory
        assert set(phase.tolist()) == {0, 1}, name
        assert (((20 * ln - phase) & 1) == phase).all()               # the odd tail occurs exactly when the phase is 1
        lens |= set(ln.tolist())
    assert lens == {4, 5, 7, 8, 9, 11, 15, 16}                        # 4: the tips of hub15's thin tets


@pytest.mark.parametrize("opts", EVQ_OPTS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("pv", ["shipped", "full"])
@pytest.mark.parametrize("name", MESHES)
def test_parity_on_a_new_state(oracle, name, pv, opts):
    """assemble on state A, then on B: the second launch leaves the a rows (shipped: uptake = 0) or writes them (full: uptake != 0,
    where they depend on the state), and the whole system is the oracle's of B either way"""
    conn, xyz = _mesh(name)
    ref = _oracle(oracle, name, pv, {}, 1)
    p = _params(pv)
    with AssemblyContext(0) as ctx:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.mesh_upload(4, conn, xyz, 5)
        ctx.field_upload(FIELD_OLD_SOLUTION, _state(xyz, 0))
        ctx.assemble_pihna(p)
        ctx.field_upload(FIELD_OLD_SOLUTION, _state(xyz, 1))
        ctx.assemble_pihna(p)
        rp, col = ctx.csr_pattern()
        np.testing.assert_array_equal(rp, ref[0])
        np.testing.assert_array_equal(col, ref[1])
        _expect(ctx, ref, f"{name} {pv} {opts} state B")
        ctx.field_upload(FIELD_OLD_SOLUTION, _state(xyz, 2))
        ctx.assemble_pihna(p)
        _expect(ctx, _oracle(oracle, name, pv, {}, 2), f"{name} {pv} {opts} state C")


@pytest.mark.parametrize("opts", [{"ev_resident": 2}, {"ev_resident": 0}], ids=["evq", "ev"])
@pytest.mark.parametrize("name", MESHES)
def test_the_skip_happens_and_only_then(oracle, name, opts):
    conn, xyz = _mesh(name)
    p = _params()
    ref_b = _oracle(oracle, name, "shipped", {}, 1)
    rp = ref_b[0]
    a_rows = _a_rows(rp)
    node = xyz.shape[0] // 2
    other = np.zeros_like(a_rows)
    other[rp[5 * node + 2]:rp[5 * node + 3]] = True                  # one row that is not an a row
    import torch
    with AssemblyContext(0) as ctx:
        for k, v in opts.items():
            ctx.set_option(k, v)
        for bad in (-1, 3):
            with pytest.raises(Exception, match="const_rows must be 0"):
                ctx.set_option("const_rows", bad)
        ctx.set_option("const_rows", 2)
        ctx.mesh_upload(4, conn, xyz, 5)
        ctx.field_upload(FIELD_OLD_SOLUTION, _state(xyz, 0))
        ctx.assemble_pihna(p)
        vt = _values_tensor(ctx, a_rows.size)
        poison_idx = torch.from_numpy(np.flatnonzero(a_rows | other)).to(vt.device)

        def poison():
            ctx.synchronize()
            vt[poison_idx] = SENTINEL
            torch.cuda.synchronize()

        def arm(what):
            """the record holds the shipped key over all rows and the a rows hold the sentinel: the next launch with that key would skip"""
            ctx.assemble_pihna(p)
            poison()
            ctx.assemble_pihna(p)
            val, rhs = ctx.csr_download()
            assert (val[a_rows] == SENTINEL).all(), what              # left alone ...
            assert not (val[~a_rows] == SENTINEL).any(), what         # ... and every other row written
            return val, rhs

        # the skip: everything but the a rows is the oracle's of the new state, the rhs of the a equation included
        poison()
        ctx.field_upload(FIELD_OLD_SOLUTION, _state(xyz, 1))
        ctx.assemble_pihna(p)
        val, rhs = ctx.csr_download()
        assert (val[a_rows] == SENTINEL).all()
        assert not (val[~a_rows] == SENTINEL).any()
        assert_csr_close(rp, ref_b[1], np.where(a_rows, ref_b[2], val), ref_b[2], rhs, ref_b[3], 5)
        assert rel(rhs, ref_b[3]) < TOL

        # ... and only then: each of these writes all five rows
        for what, changes in (("time_step", {"time_step": 0.05}), ("decay/a", {"decay/a": 1234.5}), ("uptake/a/from/v", {"uptake/a/from/v": 1.0e-5})):
            arm(what)
            ctx.assemble_pihna(_params(**changes))
            _expect(ctx, _oracle(oracle, name, "shipped", changes, 1), f"{name} {opts} changed {what}")
        arm("rdc_mesh_update_coords")
        ctx.mesh_update_coords(_moved(xyz))
        ctx.assemble_pihna(p)
        ref_m = _oracle(oracle, name, "shipped", {}, 1, moved=True)
        _expect(ctx, ref_m, f"{name} {opts} moved mesh")
        ctx.mesh_update_coords(xyz)
        arm("kernel 5")
        ctx.set_option("kernel", 5)                                   # the pair kernel writes everything ...
        ctx.assemble_pihna(p)
        _expect(ctx, ref_b, f"{name} {opts} pair kernel")
        poison()
        ctx.set_option("kernel", 0)                                   # ... and what it wrote is not the element-visit launches' to keep
        ctx.assemble_pihna(p)
        _expect(ctx, ref_b, f"{name} {opts} back from the pair kernel")
        arm("const_rows 0")
        ctx.set_option("const_rows", 0)
        ctx.assemble_pihna(p)
        _expect(ctx, ref_b, f"{name} {opts} const_rows 0")
        ctx.set_option("const_rows", 2)
        arm("const_rows 1")
        ctx.set_option("const_rows", 1)                               # the default: the value pointer is in this test's hands
        ctx.assemble_pihna(p)
        _expect(ctx, ref_b, f"{name} {opts} const_rows 1 after the pointer hand-out")
        poison()
        ctx.assemble_pihna(p)
        _expect(ctx, ref_b, f"{name} {opts} const_rows 1, again")


@pytest.mark.parametrize("resident", [0, 2])
def test_two_parts_on_two_streams(oracle, resident):
    """K(6) split in two; each rank's part 1 and part 2 on two streams with the joins of a step, twice with a new state in between
    (the second step skips), then part 1 alone with a new dt followed by a whole assembly (part 2's a rows still hold the old dt's)"""
    import torch
    conn, xyz = _mesh("k6")
    part = partition.partition_rcb(xyz[conn].mean(axis=1), 2)
    p, p_dt = _params(), _params(time_step=0.05)
    main_s, side_s = torch.cuda.current_stream(), torch.cuda.Stream()
    for rank in range(2):
        lp = partition.build_local(conn, xyz, part, rank, 2)
        assert 0 < lp.n_interior < lp.n_owned < lp.node_global.size
        lu = [_state(xyz, s)[lp.node_global] for s in (0, 1, 2)]
        ref = lambda q, s: oracle.assemble(0, 4, lp.conn, lp.xyz, 5, q, u_old=lu[s], n_owned=lp.n_owned)

        def step(q):
            side_s.wait_stream(main_s)
            ctx.assemble_pihna_part(q, 1, main_s.cuda_stream)
            ctx.assemble_pihna_part(q, 2, side_s.cuda_stream)
            main_s.wait_stream(side_s)

        with AssemblyContext(0) as ctx:
            ctx.set_stream(main_s.cuda_stream)
            ctx.set_option("ev_resident", resident)
            ctx.set_option("const_rows", 2)
            ctx.set_option("interior_nodes", int(lp.n_interior))
            ctx.mesh_upload(4, lp.conn, lp.xyz, 5, n_owned=lp.n_owned)
            rp = ctx.csr_pattern()[0]
            a_rows = _a_rows(rp)
            vt = _values_tensor(ctx, a_rows.size)
            for s in (0, 1):
                ctx.field_upload(FIELD_OLD_SOLUTION, lu[s])
                step(p)
                _expect(ctx, ref(p, s), f"rank {rank} resident {resident} step {s}")
            # the second step left the a rows of both parts: a third one shows it
            ctx.synchronize()
            vt[torch.from_numpy(np.flatnonzero(a_rows)).to(vt.device)] = SENTINEL
            torch.cuda.synchronize()
            step(p)
            val, _ = ctx.csr_download()
            assert (val[a_rows] == SENTINEL).all() and not (val[~a_rows] == SENTINEL).any()
            # part 1 alone with a new dt, then the whole mesh with it
            ctx.field_upload(FIELD_OLD_SOLUTION, lu[2])
            ctx.assemble_pihna_part(p_dt, 1, main_s.cuda_stream)
            ctx.assemble_pihna(p_dt)
            _expect(ctx, ref(p_dt, 2), f"rank {rank} resident {resident} part 1 then whole, new dt")
            step(p_dt)
            _expect(ctx, ref(p_dt, 2), f"rank {rank} resident {resident} two parts, new dt again")


def test_a_captured_launch_writes_every_row(oracle):
    """both parts captured into a graph (bench.py, two_part_host_cost); a dt change is assembled outside the graph, the a rows are
    poisoned, and the replay restores the system of the captured parameters: a captured launch never skips"""
    import torch
    conn, xyz = _mesh("k6")
    n_int = int(0.9 * xyz.shape[0])
    p, p_dt = _params(), _params(time_step=0.05)
    ref_b, ref_dt = _oracle(oracle, "k6", "shipped", {}, 1), _oracle(oracle, "k6", "shipped", {"time_step": 0.05}, 1)
    a_rows = _a_rows(ref_b[0])
    with AssemblyContext(0) as ctx:
        ctx.set_option("const_rows", 2)
        ctx.set_option("ev_resident", 2)
        ctx.set_option("interior_nodes", n_int)
        ctx.mesh_upload(4, conn, xyz, 5)
        u_t = torch.from_numpy(_state(xyz, 0)).to("cuda:0")
        ctx.field_bind_device(FIELD_OLD_SOLUTION, u_t.data_ptr(), u_t.numel())
        vt = _values_tensor(ctx, a_rows.size)
        a_idx = torch.from_numpy(np.flatnonzero(a_rows)).to(vt.device)
        for _ in range(2):                                            # the record is set: a launch outside a graph would skip now
            ctx.assemble_pihna_part(p, 1, 0)
            ctx.assemble_pihna_part(p, 2, 0)
        g = torch.cuda.CUDAGraph()
        cap_s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=cap_s):
            ctx.assemble_pihna_part(p, 1, cap_s.cuda_stream)
            ctx.assemble_pihna_part(p, 2, cap_s.cuda_stream)
        torch.cuda.synchronize()
        u_t.copy_(torch.from_numpy(_state(xyz, 1)))
        ctx.assemble_pihna(p_dt)                                      # outside the graph: the a rows now hold the other dt's values
        _expect(ctx, ref_dt, "new dt outside the graph")
        ctx.synchronize()
        vt[a_idx] = SENTINEL
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _expect(ctx, ref_b, "replay")
        # the replay put the captured dt's rows back behind the host's back: a launch with the other dt may not trust its record
        ctx.assemble_pihna(p_dt)
        _expect(ctx, ref_dt, "new dt after the replay")
        ctx.assemble_pihna(p)
        ctx.synchronize()
        vt[a_idx] = SENTINEL
        torch.cuda.synchronize()
        ctx.assemble_pihna(p)                                         # the captured key itself may still be skipped
        val, _ = ctx.csr_download()
        assert (val[a_rows] == SENTINEL).all() and not (val[~a_rows] == SENTINEL).any()
