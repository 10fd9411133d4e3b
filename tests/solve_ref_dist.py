"""numpy yardstick of the partitioned BiCGStab (rdc_solve_dist; rdcfes_amd/csrc/rdc_solve.hip with a communicator): the iteration of
solve_ref.bicgstab, restated on what the ranks hold.  Every rank has the rows of its owned nodes over its LOCAL dofs (owned
first, ghosts behind them, grouped by owner: partition.build_local), assembled by the oracle with n_owned as
solve_systems.ghosted_pihna does; an operator application fills the ghost tail of its argument from the owners through the
send lists (lp.send_ids -> the peer's lp.recv_ids) and multiplies locally; every inner product is the sum, in rank order, of
the ranks' own sums; every decision is taken on those global sums, once, for all ranks.

bicgstab_dist is a thin driver of the shape of solve_ref.bicgstab rather than a call of it: that driver's inner products are
single `@`s over one vector, and the point here is the rank-wise sum.  split() gives the ranks of a solve_systems.System."""
import copy
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sps

import solve_ref
import solve_systems
from rdcfes_amd import partition
from solve_ref import BREAKDOWN, CONVERGED, MAX_BREAKDOWNS, MAX_ITS, NOT_FINITE


@dataclass
class Rank:
    lp: object            # partition.LocalPartition
    system: object        # the local solve_systems.System (local conn / xyz / fields, n_owned)
    A: object = None      # [n_owned * nv][n_local * nv], local numbering
    b: np.ndarray = None


# the systems the partitioned tests run on: K(8) PIHNA and the jittered HEX8 HCC of solve_systems, and K(3): 64 nodes, where a rank of
# three owns fewer rows than one SpMV workgroup has and has no interior at all
CASES = {"pihna_kuhn": lambda: solve_systems.get("pihna_kuhn"), "hcc_hex": lambda: solve_systems.get("hcc_hex"),
         "pihna_kuhn3": lambda: solve_systems.pihna_kuhn(3)}
_CASE, _GLOBAL, _SPLIT, _YARD = {}, {}, {}, {}


def case(name):
    if name not in _CASE:
        _CASE[name] = CASES[name]()
    return _CASE[name]


def global_system(name, O):
    """(System, A, b) of the oracle's global assembly, b = rhs_scale * rhs; computed once and not to be modified"""
    if name not in _GLOBAL:
        s = case(name)
        rp, col, val, rhs = s.oracle_assemble(O)
        _GLOBAL[name] = (s, sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size)), s.rhs_scale * rhs)
    return _GLOBAL[name]


def ranks_of(name, world, O):
    if (name, world) not in _SPLIT:
        _SPLIT[(name, world)] = split(case(name), world, O)
    return _SPLIT[(name, world)]


def yardstick(name, O, rel_tol, precond=2):
    """info of solve_ref.bicgstab on the global system from x0 = 0; computed once"""
    if (name, rel_tol, precond) not in _YARD:
        s, A, b = global_system(name, O)
        _YARD[(name, rel_tol, precond)] = solve_ref.bicgstab(A, b, np.zeros(b.size), rel_tol, precond=precond, nv=s.nv)
    return _YARD[(name, rel_tol, precond)]


def local_system(s, lp):
    """the System of one rank: local mesh, the fields of its nodes, rows = its owned nodes"""
    loc = copy.copy(s)
    loc.name = f"{s.name}_r{lp.rank}of{lp.nparts}"
    loc.conn, loc.xyz, loc.n_owned = lp.conn, lp.xyz, lp.n_owned
    loc.fields = {f: np.ascontiguousarray(np.asarray(a)[lp.node_global]) for f, a in s.fields.items()}
    return loc


def partitions(s, world):
    """[LocalPartition] of every rank: recursive coordinate bisection of the element centroids, as bench.py partitions"""
    part = partition.partition_rcb(s.xyz[s.conn.astype(np.int64)].mean(axis=1), world)
    owner = partition.node_owners(s.conn, part, s.xyz.shape[0], world)
    return [partition.build_local(s.conn, s.xyz, part, r, world, owner=owner) for r in range(world)]


def split(s, world, O):
    """[Rank] with the oracle's local assemblies"""
    out = []
    for lp in partitions(s, world):
        loc = local_system(s, lp)
        rp, col, val, rhs = loc.oracle_assemble(O)
        A = sps.csr_matrix((val, col, rp), shape=(lp.n_owned * s.nv, lp.xyz.shape[0] * s.nv))
        out.append(Rank(lp, loc, A, s.rhs_scale * rhs))
    return out


def interior_rows_read_no_ghost(rk, nv):
    """every column of a row below n_interior is an owned dof"""
    A = rk.A.tocsr()
    cols = A.indices[:A.indptr[rk.lp.n_interior * nv]]
    return cols.size == 0 or int(cols.max()) < rk.lp.n_owned * nv


def exchange(ranks, vecs, nv):
    """ghost tails of the ranks' local vectors (each [n_local * nv]) from the owners, through the send lists"""
    for rk, v in zip(ranks, vecs):
        for q, ids in rk.lp.recv_ids.items():
            src = ranks[q].lp.send_ids[rk.lp.rank]
            v.reshape(-1, nv)[ids] = vecs[q].reshape(-1, nv)[src]


def gather(ranks, vecs, nv, n_node):
    """global vector from the owned rows of the local ones"""
    x = np.full((n_node, nv), np.nan)
    for rk, v in zip(ranks, vecs):
        x[rk.lp.node_global[:rk.lp.n_owned]] = v.reshape(-1, nv)[:rk.lp.n_owned]
    return x.reshape(-1)


def bicgstab_dist(ranks, x0s, rel_tol, abs_tol=0.0, max_its=10000, precond=2, nv=1):
    """x0s: per rank [n_local * nv] (ghost entries ignored).  -> (xs, info): xs per rank over local dofs, ghost tails filled by
    the last exchange of x; info as solve_ref.bicgstab's, every figure global"""
    R = range(len(ranks))
    no = [rk.lp.n_owned * nv for rk in ranks]
    # D^-1 of the owned rows: the diagonal blocks lie in the leading square of a rank's rows
    M = [solve_ref.precond_inverse(rk.A[:, :n].tocsr(), nv, precond)[0] for rk, n in zip(ranks, no)]
    xs = [np.array(x, dtype=np.float64, copy=True) for x in x0s]
    dot = lambda a, b: float(sum(float(a[r] @ b[r]) for r in R))   # rank-wise, then over the ranks in order

    def full(owned):     # owned parts -> local vectors with a ghost tail to receive into
        return [np.concatenate([owned[r], np.zeros(ranks[r].A.shape[1] - no[r])]) for r in R]

    def A_of(vecs):      # exchange, then every rank's rows
        exchange(ranks, vecs, nv)
        return [ranks[r].A @ vecs[r] for r in R]

    def operator(owned):
        ax = A_of(full(owned))
        return [M[r] @ ax[r] for r in R]

    info = dict(reason=CONVERGED, iterations=0, restarts=0)
    mb = [M[r] @ ranks[r].b for r in R]
    bn = float(np.sqrt(dot(mb, mb)))
    info["rhs_norm"] = bn

    def restart():
        ax = A_of(xs)
        r_ = [M[r] @ (ranks[r].b - ax[r]) for r in R]
        z = [np.zeros_like(v) for v in r_]
        return r_, [v.copy() for v in r_], z, [v.copy() for v in z], dot(r_, r_), 1.0, 1.0, 0.0

    def done(reason, rn2):
        info["reason"], info["residual_norm"] = reason, float(np.sqrt(rn2))
        return xs, info

    r_, rh, p, v, rn2, alpha, omega, beta = restart()
    rho = rn2
    if not (np.isfinite(bn) and np.isfinite(rn2)):
        return done(NOT_FINITE, rn2)
    if bn == 0.0:
        for x in xs:
            x[:] = 0.0
        return done(CONVERGED, 0.0)
    tol = max(rel_tol * bn, abs_tol)
    if np.sqrt(rn2) <= tol:
        return done(CONVERGED, rn2)
    breakdowns = 0
    while True:
        if info["iterations"] >= max_its:
            _, _, _, _, rn2, _, _, _ = restart()
            return done(CONVERGED if np.sqrt(rn2) <= tol else MAX_ITS, rn2)
        info["iterations"] += 1
        flag = 0
        with np.errstate(all="ignore"):
            p = [r_[r] + beta * (p[r] - omega * v[r]) for r in R]
            v = operator(p)
            r0v = dot(rh, v)
            alpha = rho / r0v if r0v != 0.0 else np.inf
            if r0v == 0.0 or not np.isfinite(alpha):
                flag = 1
            if not flag:
                s = [r_[r] - alpha * v[r] for r in R]
                t = operator(s)
                ts, tt = dot(t, s), dot(t, t)
                omega = ts / tt if tt > 0.0 else 0.0
                if omega == 0.0 or not np.isfinite(omega):
                    flag = 1
            if not flag:
                for r in R:
                    xs[r][:no[r]] += alpha * p[r] + omega * s[r]
                r_ = [s[r] - omega * t[r] for r in R]
                rho1, rn2 = dot(rh, r_), dot(r_, r_)
                beta = (rho1 / rho) * (alpha / omega)
                rho = rho1
                if not (np.isfinite(rn2) and np.isfinite(beta)):
                    flag = 1
                elif rho1 == 0.0:
                    flag = 2
        claims = not (flag & 1) and np.sqrt(rn2) <= tol
        if not claims and not flag:
            continue
        if not claims:
            breakdowns += 1
        r_, rh, p, v, rn2, alpha, omega, beta = restart()
        rho = rn2
        if not claims and breakdowns > MAX_BREAKDOWNS:
            return done(BREAKDOWN if np.isfinite(rn2) else NOT_FINITE, rn2)
        if not np.isfinite(rn2):
            return done(NOT_FINITE, rn2)
        if np.sqrt(rn2) <= tol:
            return done(CONVERGED, rn2)
        info["restarts"] += 1
