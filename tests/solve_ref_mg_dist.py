"""numpy yardstick of the multigrid solve across ranks (rdc_solve_dist_mg; rdc_solve.h: mg_dist_aggregate / mg_dist_coarsen,
rdc_solve.hip: the cycle with a communicator), restated on what the ranks hold, as solve_ref_dist restates block Jacobi.

Hierarchy (per rank, per level): the aggregation of solve_ref_mg on the edges whose two ends the rank owns; one exchange of
aggregate numbers along the level's send lists; the coarse ghosts from peer q are the distinct numbers received in q's ghost
segment, in order of first appearance, numbered behind the owned aggregates in peer order; the coarse send segment for q is the
distinct own aggregates of the fine send segment for q, in order of first appearance.  Levels are added until the level has at
most COARSEST_NODES nodes over all ranks, MAX_LEVELS exist or no rank merged anything.  Peers of a rank: every rank it sends to
or receives from, ascending (halo.SolveComm.peers).

Cycle and iteration: solve_ref_mg's V(1,1) cycle and right-preconditioned BiCGStab with every operator application preceded by
the exchange of its argument on that level and every inner product summed rank by rank, as solve_ref_dist.bicgstab_dist does.

emulate(): the same method as ONE global solve_ref_mg.Hierarchy whose nodes are ordered rank by rank on every level -- what the
ranks together compute, without any exchange; the two must agree to rounding."""
import numpy as np
import scipy.sparse as sps

import solve_ref
import solve_ref_dist
import solve_ref_mg
from solve_ref import BREAKDOWN, CONVERGED, MAX_BREAKDOWNS, MAX_ITS, NOT_FINITE
from solve_ref_mg import COARSEST_NODES, COARSEST_SWEEPS, MAX_LEVELS, OMEGA


def peers_of(lp):
    return sorted(set(lp.send_ids) | set(lp.recv_ids))


def first_appearance(ids):
    """the distinct entries of ids in order of first appearance, and the position of every entry in that list"""
    uniq, first, inv = np.unique(ids, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return uniq[order], rank[inv.reshape(-1)]


def slots(n_owned, send_nodes):
    """(send_ptr, send_slot): the positions of every owned node in the send list, ascending"""
    ptr = np.concatenate([[0], np.cumsum(np.bincount(send_nodes, minlength=n_owned))]).astype(np.int64)
    return ptr, np.argsort(send_nodes, kind="stable").astype(np.int32)


def halo0(lp):
    """level 0 of a rank: dict(n, n_ghost, peers, send_off, ghost_off, send_nodes, send_ptr, send_slot), offsets in nodes"""
    peers = peers_of(lp)
    sc = [len(lp.send_ids.get(q, ())) for q in peers]
    gc = [len(lp.recv_ids.get(q, ())) for q in peers]
    send = np.concatenate([np.asarray(lp.send_ids.get(q, ()), dtype=np.int32) for q in peers] + [np.zeros(0, np.int32)]).astype(np.int32)
    ptr, slot = slots(lp.n_owned, send)
    return dict(n=lp.n_owned, n_ghost=lp.xyz.shape[0] - lp.n_owned, peers=peers, send_off=np.concatenate([[0], np.cumsum(sc)]).astype(np.int64),
                ghost_off=np.concatenate([[0], np.cumsum(gc)]).astype(np.int64), send_nodes=send, send_ptr=ptr, send_slot=slot)


def owned_pattern(bptr, bcol, n):
    keep = bcol < n
    rows = np.repeat(np.arange(n), np.diff(bptr))
    return np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int64), bcol[keep]


def exchange_ids(halos, sends):
    """per rank the ghost tail of the values its peers send it: segment k of rank r's tail = the segment peer k keeps for r"""
    out = []
    for r, H in enumerate(halos):
        tail = np.full(H["n_ghost"], -1.0)
        for k, q in enumerate(H["peers"]):
            Q = halos[q]
            j = Q["peers"].index(r)
            seg = sends[q][Q["send_off"][j]:Q["send_off"][j + 1]]
            assert seg.size == H["ghost_off"][k + 1] - H["ghost_off"][k]
            tail[H["ghost_off"][k]:H["ghost_off"][k + 1]] = seg
        out.append(tail)
    return out


def coarsen(H, bptr, bcol, agg, na, ids_in):
    """one rank's step behind the exchange -> (step dict(agg [n + n_ghost], n, bptr, bcol, cptr, cidx), coarse halo)"""
    full = np.concatenate([agg, np.zeros(H["n_ghost"], dtype=np.int32)]).astype(np.int32)
    nxt, goff, soff, send = na, [0], [0], []
    for k in range(len(H["peers"])):
        g0, g1 = H["ghost_off"][k], H["ghost_off"][k + 1]
        uniq, pos = first_appearance(ids_in[g0:g1].astype(np.int64))
        full[H["n"] + g0:H["n"] + g1] = nxt + pos
        nxt += uniq.size
        goff.append(nxt - na)
        mine, _ = first_appearance(agg[H["send_nodes"][H["send_off"][k]:H["send_off"][k + 1]]])
        send.append(mine.astype(np.int32))
        soff.append(soff[-1] + mine.size)
    send = np.concatenate(send + [np.zeros(0, np.int32)]).astype(np.int32)
    ncols = nxt
    rows = np.repeat(np.arange(H["n"]), np.diff(bptr))
    key = full[rows].astype(np.int64) * ncols + full[bcol]
    uniq, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    cb = np.zeros(na + 1, dtype=np.int64)
    np.add.at(cb, uniq // ncols + 1, 1)
    cptr = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=uniq.size))]).astype(np.int64)
    ptr, slot = slots(na, send)
    step = dict(agg=full, n=na, bptr=np.cumsum(cb), bcol=(uniq % ncols).astype(np.int32), cptr=cptr, cidx=np.argsort(inv, kind="stable").astype(np.int32))
    C = dict(n=na, n_ghost=nxt - na, peers=H["peers"], send_off=np.array(soff, dtype=np.int64), ghost_off=np.array(goff, dtype=np.int64),
             send_nodes=send, send_ptr=ptr, send_slot=slot)
    return step, C


def pattern_hierarchy_dist(patterns, lps):
    """patterns: per rank (bptr, bcol) of the owned rows over local nodes.  -> (steps, halos, ids): steps[r][l] takes level l to
    l + 1 on rank r, halos[r][l] is the ghost layer of level l, ids[r][l] = (sent, received) aggregate numbers of step l"""
    R = range(len(lps))
    halos = [[halo0(lp)] for lp in lps]
    steps, ids = [[] for _ in R], [[] for _ in R]
    pats = [(np.asarray(b, dtype=np.int64), np.asarray(c, dtype=np.int32)) for b, c in patterns]
    while True:
        H = [halos[r][-1] for r in R]
        aggs = [solve_ref_mg.aggregate(*owned_pattern(*pats[r], H[r]["n"])) for r in R]
        nodes, merged = sum(h["n"] for h in H), sum(int(a[1] < h["n"]) for a, h in zip(aggs, H))
        if not (nodes > COARSEST_NODES and len(halos[0]) < MAX_LEVELS and merged > 0):
            return steps, halos, ids
        sends = [aggs[r][0][H[r]["send_nodes"]].astype(np.float64) for r in R]
        recvs = exchange_ids(H, sends)
        for r in R:
            st, C = coarsen(H[r], *pats[r], aggs[r][0], aggs[r][1], recvs[r])
            st["n_pass1"] = aggs[r][2]
            steps[r].append(st)
            halos[r].append(C)
            ids[r].append((sends[r], recvs[r]))
            pats[r] = (st["bptr"], st["bcol"])


class HierarchyDist:
    """the levels of every rank with their values: lv[r][l] = dict(n, n_ghost, blocks, A [n nv][(n + n_ghost) nv], Dinv, P)"""

    def __init__(self, ranks, nv, omega=OMEGA):
        self.nv, self.omega, self.ranks = nv, omega, ranks
        R = range(len(ranks))
        self.M0, self.lv, pats = [], [[] for _ in R], []
        for r, rk in enumerate(ranks):
            n = rk.lp.n_owned
            bptr, bcol, blocks = solve_ref_mg.block_pattern(sps.csr_matrix(rk.A), nv)
            M, Di, _ = solve_ref.precond_inverse(rk.A[:, :n * nv].tocsr(), nv, 2)
            self.M0.append(M)
            rows = np.repeat(np.arange(n), np.diff(bptr))
            self.lv[r].append(dict(n=n, n_ghost=rk.lp.xyz.shape[0] - n, blocks=solve_ref_mg.scaled_blocks(Di[rows], blocks)))
            pats.append((bptr, bcol))
        self.steps, self.halos, self.ids = pattern_hierarchy_dist(pats, [rk.lp for rk in ranks])
        for r in R:
            for l, st in enumerate(self.steps[r]):
                fine, H = self.lv[r][l], self.halos[r][l + 1]
                agg = st["agg"][:fine["n"]]
                fine["P"] = sps.kron(sps.csr_matrix((np.ones(agg.size), agg, np.arange(agg.size + 1)), shape=(agg.size, st["n"])), sps.eye(nv)).tocsr()
                blocks = solve_ref_mg.galerkin(fine["blocks"], st["cptr"], st["cidx"])
                shape = (st["n"] * nv, (st["n"] + H["n_ghost"]) * nv)
                A = sps.bsr_matrix((blocks, st["bcol"], st["bptr"]), shape=shape).tocsr() if st["n"] else sps.csr_matrix(shape)
                Dinv = solve_ref.precond_inverse(A[:, :st["n"] * nv].tocsr(), nv, 2)[0] if st["n"] else sps.csr_matrix((0, 0))
                self.lv[r].append(dict(n=st["n"], n_ghost=H["n_ghost"], blocks=blocks, A=A, Dinv=Dinv))
        self.n_levels = len(self.lv[0])
        self.exchanges = [0] * self.n_levels     # per level, counted once per collective exchange

    def level_sizes(self, r):
        """[(owned nodes, node blocks of the rank's rows)] per level"""
        b0 = solve_ref_mg.block_pattern(sps.csr_matrix(self.ranks[r].A), self.nv)[1].size
        return [(self.lv[r][0]["n"], b0)] + [(st["n"], st["bcol"].size) for st in self.steps[r]]

    def _exchange(self, l, vecs):
        self.exchanges[l] += 1
        nv = self.nv
        H = [self.halos[r][l] for r in range(len(vecs))]
        sends = [vecs[r].reshape(-1, nv)[H[r]["send_nodes"]] for r in range(len(vecs))]
        for r, v in enumerate(vecs):
            for k, q in enumerate(H[r]["peers"]):
                j = H[q]["peers"].index(r)
                v.reshape(-1, nv)[H[r]["n"] + H[r]["ghost_off"][k]:H[r]["n"] + H[r]["ghost_off"][k + 1]] = \
                    sends[q][H[q]["send_off"][j]:H[q]["send_off"][j + 1]]

    def op(self, l, owned):
        """the level's operator on the ranks' owned parts: ghost tails from the owners, then every rank's rows"""
        R = range(len(owned))
        full = [np.concatenate([owned[r], np.zeros(self.lv[r][l]["n_ghost"] * self.nv)]) for r in R]
        self._exchange(l, full)
        if l == 0:
            return [self.M0[r] @ (self.ranks[r].A @ full[r]) for r in R]
        return [self.lv[r][l]["A"] @ full[r] for r in R]

    def _smooth(self, l, res):
        if l == 0:
            return [self.omega * v for v in res]
        return [self.omega * (self.lv[r][l]["Dinv"] @ v) for r, v in enumerate(res)]

    def cycle(self, rs, l=0):
        R = range(len(rs))
        sub = lambda a, b: [a[r] - b[r] for r in R]
        add = lambda a, b: [a[r] + b[r] for r in R]
        x = self._smooth(l, rs)
        if l == self.n_levels - 1:
            for _ in range(COARSEST_SWEEPS - 1):
                x = add(x, self._smooth(l, sub(rs, self.op(l, x))))
            return x
        P = [self.lv[r][l]["P"] for r in R]
        res = sub(rs, self.op(l, x))
        xc = self.cycle([P[r].T @ res[r] for r in R], l + 1)
        x = add(x, [P[r] @ xc[r] for r in R])
        return add(x, self._smooth(l, sub(rs, self.op(l, x))))


def bicgstab_dist(ranks, x0s, rel_tol, abs_tol=0.0, max_its=10000, nv=1, hierarchy=None):
    """solve_ref_dist.bicgstab_dist(precond=2) with the cycle applied from the right -> (xs, info); info also has n_levels and
    level_exchanges (per level, of the whole solve)"""
    H = hierarchy or HierarchyDist(ranks, nv)
    R = range(len(ranks))
    no = [rk.lp.n_owned * nv for rk in ranks]
    M = H.M0
    xs = [np.array(x, dtype=np.float64, copy=True) for x in x0s]
    dot = lambda a, b: float(sum(float(a[r] @ b[r]) for r in R))
    info = dict(reason=CONVERGED, iterations=0, restarts=0, n_levels=H.n_levels)
    mb = [M[r] @ ranks[r].b for r in R]
    bn = float(np.sqrt(dot(mb, mb)))
    info["rhs_norm"] = bn

    def restart():
        solve_ref_dist.exchange(ranks, xs, nv)
        r_ = [M[r] @ (ranks[r].b - ranks[r].A @ xs[r]) for r in R]
        z = [np.zeros_like(v) for v in r_]
        return r_, [v.copy() for v in r_], z, [v.copy() for v in z], dot(r_, r_), 1.0, 1.0, 0.0

    def done(reason, rn2):
        info["reason"], info["residual_norm"], info["level_exchanges"] = reason, float(np.sqrt(rn2)), list(H.exchanges)
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
            ph = H.cycle(p)
            v = H.op(0, ph)
            r0v = dot(rh, v)
            alpha = rho / r0v if r0v != 0.0 else np.inf
            if r0v == 0.0 or not np.isfinite(alpha):
                flag = 1
            if not flag:
                s = [r_[r] - alpha * v[r] for r in R]
                sh = H.cycle(s)
                t = H.op(0, sh)
                ts, tt = dot(t, s), dot(t, t)
                omega = ts / tt if tt > 0.0 else 0.0
                if omega == 0.0 or not np.isfinite(omega):
                    flag = 1
            if not flag:
                for r in R:
                    xs[r][:no[r]] += alpha * ph[r] + omega * sh[r]
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


class EmulatedHierarchy(solve_ref_mg.Hierarchy):
    """ONE global hierarchy with rank-local aggregates.  A: the global matrix with its nodes ordered rank by rank, each rank's in
    its local owned order; counts[r] = nodes of rank r.  On every level the nodes stay ordered rank by rank (a rank's aggregates in
    its own numbering), and an aggregate only takes nodes of one rank."""

    def __init__(self, A, nv, counts, omega=OMEGA):
        self.nv, self.omega = nv, omega
        bptr, bcol, blocks = solve_ref_mg.block_pattern(A, nv)
        n = bptr.size - 1
        rows = np.repeat(np.arange(n), np.diff(bptr))
        M0, Di, _ = solve_ref.precond_inverse(A, nv, 2)
        lv = dict(n=n, bptr=bptr, bcol=bcol, blocks=solve_ref_mg.scaled_blocks(Di[rows], blocks))
        self.M0, self.A0, self.levels, self.counts = M0, A, [lv], [list(counts)]
        counts = list(counts)
        while n > COARSEST_NODES and len(self.levels) < MAX_LEVELS:
            agg, new_counts, o, merged = np.empty(n, dtype=np.int32), [], 0, 0
            for c in counts:
                rows = np.repeat(np.arange(n), np.diff(bptr))
                keep = (rows >= o) & (rows < o + c) & (bcol >= o) & (bcol < o + c)
                sp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep] - o, minlength=c))]).astype(np.int64)
                a, na, _, _ = solve_ref_mg.aggregate(sp, (bcol[keep] - o).astype(np.int32))
                agg[o:o + c] = a + sum(new_counts)
                merged += int(na < c)
                new_counts.append(na)
                o += c
            if not merged:
                break
            na = sum(new_counts)
            cb, cc, cptr, cidx = solve_ref_mg.coarse_pattern(bptr, bcol, agg, na)
            lv["agg"] = agg
            lv["P"] = sps.kron(sps.csr_matrix((np.ones(n), agg, np.arange(n + 1)), shape=(n, na)), sps.eye(nv)).tocsr()
            lv = dict(n=na, bptr=cb, bcol=cc, blocks=solve_ref_mg.galerkin(lv["blocks"], cptr, cidx), cptr=cptr, cidx=cidx)
            self.levels.append(lv)
            self.counts.append(new_counts)
            n, bptr, bcol, counts = na, cb, cc, new_counts
        for l, lv in enumerate(self.levels):
            if l:
                N = lv["n"] * nv
                lv["A"] = sps.bsr_matrix((lv["blocks"], lv["bcol"], lv["bptr"]), shape=(N, N)).tocsr()
                lv["Dinv"] = solve_ref.precond_inverse(lv["A"], nv, 2)[0]


def rank_order(ranks):
    """global node of every position of the rank-by-rank order, and the nodes per rank"""
    return np.concatenate([rk.lp.node_global[:rk.lp.n_owned] for rk in ranks]), [rk.lp.n_owned for rk in ranks]


def emulate(A, b, ranks, nv, rel_tol):
    """the global emulation from x0 = 0 -> (x in the global numbering, info, hierarchy)"""
    perm, counts = rank_order(ranks)
    dof = (perm[:, None] * nv + np.arange(nv)).reshape(-1)
    Ap = sps.csr_matrix(A)[dof][:, dof].tocsr()
    H = EmulatedHierarchy(Ap, nv, counts)
    xp, info = solve_ref_mg.bicgstab(Ap, b[dof], np.zeros(b.size), rel_tol, nv=nv, hierarchy=H)
    x = np.empty_like(xp)
    x[dof] = xp
    return x, info, H
