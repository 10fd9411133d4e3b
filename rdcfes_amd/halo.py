"""Halo exchange of ghost-node DoFs (`system.update()` of the reference, src/pihna.C:801;
SURVEY §2.3, §8e) with torch.distributed: backend "nccl" is RCCL over xGMI on MI355X, "gloo" on CPU
for the tests.  One grouped point-to-point round per step (each GPU talks to its few face
neighbours over its direct xGMI links; the messages are O(0.1-2 MB), latency-bound) -- no
all-reduce, no ring.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

from .params import (ALLREDUCE_SUM_FN, EXCHANGE_BEGIN_FN, EXCHANGE_END_FN, EXCHANGE_SIZED_BEGIN_FN, SolveCommSizedStruct,
                     SolveCommStruct, SolveCommWideStruct)

WIDE_MAX = 130   # doubles of the longest wide all-reduce: "gmres_restart" <= 128, and a step sums up to restart + 1 (+ 1 spare)


class HaloExchange:
    """All peers share ONE send and ONE receive buffer (per-peer slices of them are what is sent): a step costs one
    gather kernel, one grouped send/recv and one scatter kernel whatever the number of neighbours -- at 8 GPUs
    the assembly kernel is ~0.4 ms, so per-peer launches would be a visible fraction of the step."""

    def __init__(self, lp, nvar: int, device, group=None):
        self.group = group
        self.nvar = nvar
        self.rank = lp.rank
        self.peers = sorted(set(lp.send_ids) | set(lp.recv_ids))
        dev = torch.device(device)
        as_idx = lambda a: torch.as_tensor(a, dtype=torch.long, device=dev)
        self.send_peers = [q for q in self.peers if q in lp.send_ids and len(lp.send_ids[q])]
        self.recv_peers = [q for q in self.peers if q in lp.recv_ids and len(lp.recv_ids[q])]
        cat = lambda ids, qs: as_idx([i for q in qs for i in ids[q]]) if qs else as_idx([])
        self.send_idx = cat(lp.send_ids, self.send_peers)
        self.recv_idx = cat(lp.recv_ids, self.recv_peers)
        self.send_buf = torch.empty((self.send_idx.numel(), nvar), dtype=torch.float64, device=dev)
        self.recv_buf = torch.empty((self.recv_idx.numel(), nvar), dtype=torch.float64, device=dev)
        self.bytes_per_step = 8 * nvar * int(self.send_idx.numel())
        # gloo cannot move device tensors: stage through host buffers (test rigs with one GPU only;
        # the production backend is "nccl" = RCCL, which sends the device buffers directly)
        self.host_staged = dev.type == "cuda" and dist.is_initialized() and dist.get_backend(group) == "gloo"
        if self.host_staged:
            self.send_host = torch.empty_like(self.send_buf, device="cpu").pin_memory()
            self.recv_host = torch.empty_like(self.recv_buf, device="cpu").pin_memory()
        sb = self.send_host if self.host_staged else self.send_buf
        rb = self.recv_host if self.host_staged else self.recv_buf

        def views(buf, ids, qs):
            out, o = {}, 0
            for q in qs:
                n = len(ids[q])
                out[q] = buf[o:o + n]
                o += n
            return out
        self.send_view = views(sb, lp.send_ids, self.send_peers)
        self.recv_view = views(rb, lp.recv_ids, self.recv_peers)
        self._ops = None   # the P2POp list is the same every step: built once (needs the process group to exist)

    def exchange_many(self, fields):
        """Several nodal fields in ONE grouped message per peer: fields = [tensor [n_node_local][w_k], ...] with
        sum(w_k) == nvar.  The coupled HCC + solid step (BASELINE config 5) moves the HCC unknowns (3 per node) and the
        CURRENT coordinates of the moving mesh (3 per node: the solid system's solution, src/solid_system.C:103-123)
        together: the message count, not the bytes, is what a step pays for."""
        if sum(int(f.shape[1]) for f in fields) != self.nvar:
            raise ValueError("field widths do not add up to the exchange's nvar")
        if not self.send_peers and not self.recv_peers:
            return
        if self.send_idx.numel():
            o = 0
            for f in fields:
                w = int(f.shape[1])
                self.send_buf[:, o:o + w].copy_(f.index_select(0, self.send_idx))
                o += w
        self._round()
        if self.recv_idx.numel():
            o = 0
            for f in fields:
                w = int(f.shape[1])
                f.index_copy_(0, self.recv_idx, self.recv_buf[:, o:o + w])
                o += w

    def _round(self):
        """send_buf -> peers -> recv_buf (one grouped isend / irecv round)"""
        if self.send_idx.numel() and self.host_staged:
            self.send_host.copy_(self.send_buf, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        if self._ops is None:
            self._ops = [dist.P2POp(dist.irecv, self.recv_view[q], q, group=self.group) for q in self.recv_peers]
            self._ops += [dist.P2POp(dist.isend, self.send_view[q], q, group=self.group) for q in self.send_peers]
        for w in dist.batch_isend_irecv(self._ops):
            w.wait()
        if self.recv_idx.numel() and self.host_staged:
            self.recv_buf.copy_(self.recv_host, non_blocking=True)

    def exchange(self, u: torch.Tensor):
        """u: [n_node_local][nvar]; owned rows are read, ghost rows are overwritten in place."""
        if not self.send_peers and not self.recv_peers:
            return
        if self.send_idx.numel():
            torch.index_select(u, 0, self.send_idx, out=self.send_buf)
            if self.host_staged:
                self.send_host.copy_(self.send_buf, non_blocking=True)
                torch.cuda.current_stream().synchronize()
        if self._ops is None:
            self._ops = [dist.P2POp(dist.irecv, self.recv_view[q], q, group=self.group) for q in self.recv_peers]
            self._ops += [dist.P2POp(dist.isend, self.send_view[q], q, group=self.group) for q in self.send_peers]
        for w in dist.batch_isend_irecv(self._ops):
            w.wait()
        if self.recv_idx.numel():
            if self.host_staged:
                self.recv_buf.copy_(self.recv_host, non_blocking=True)
            u.index_copy_(0, self.recv_idx, self.recv_buf)


class SolveComm:
    """The communicator of AssemblyContext.solve_dist (rdc_solve_comm of the C-ABI) on torch.distributed: the three callbacks
    the library calls from inside its BiCGStab -- exchange_begin / exchange_end move the ghost values of one vector (the library
    has packed the send buffer; the ghosts are the contiguous tail of the vector, grouped by owner, so the receive side needs
    no unpack), allreduce_sum adds up to 8 doubles over the ranks.  "nccl" (RCCL) works on the device buffers, on the stream
    the library names; "gloo" stages through pinned host buffers and synchronises that stream, as HaloExchange does: a test rig,
    correct but no measure of speed.  Without an initialised process group the communicator is that of world size 1.

    send_nodes is the send list for rdc_solve_dist_plan (peer order, per peer the order of lp.send_ids, which is the order of
    the peer's lp.recv_ids: ascending global id on both sides).  An exception inside a callback is kept in .error and the
    callback returns 1; solve_dist re-raises it.  Subclasses may override begin / end / allreduce (tests do).

    sized=True adds what the multigrid solve across ranks needs (rdc_solve_comm_sized, rdc_solve_dist_mg): sized_begin / sized_end
    move the ghost values of a level below the matrix, whose per-peer slices come with the call, over ONE peer list (`peers`: every
    rank this one sends to or receives from, ascending); peer_counts are the plan's segment lengths over that list for
    rdc_solve_dist_plan_peers.  The gloo staging buffers serve them too: no level has more to move than the plan.  Without it
    solve_dist(precond=PRECOND_MULTIGRID) stays RDC_ERR_UNSUPPORTED.

    wide=True adds what GMRES across ranks needs (rdc_solve_comm_wide, AssemblyContext.solve_dist_gmres and gmres_arnoldi_dist):
    allreduce_wide adds up to 130 doubles over the ranks, the inner products of one Gram-Schmidt pass in one message.  It implies
    the sized callbacks when the plan has peers (the multigrid preconditioner needs them).  wide_allreduces counts its calls and
    wide_lengths lists the lengths it saw."""

    def __init__(self, lp, nvar: int, device, group=None, sized=False, wide=False):
        self.group, self.nvar, self.rank = group, int(nvar), lp.rank
        self.dev = torch.device(device)
        peers = sorted(set(lp.send_ids) | set(lp.recv_ids))
        sized = sized or (wide and bool(peers))
        self.send_peers = [q for q in peers if q in lp.send_ids and len(lp.send_ids[q])]
        self.recv_peers = [q for q in peers if q in lp.recv_ids and len(lp.recv_ids[q])]
        self.send_nodes = (np.concatenate([np.asarray(lp.send_ids[q]) for q in self.send_peers]) if self.send_peers
                           else np.zeros(0)).astype(np.int32)
        self.n_send, self.n_ghost = int(self.send_nodes.size), int(lp.xyz.shape[0] - lp.n_owned)
        # per-peer slices, in rows of nvar doubles: of the send buffer, and of the ghost tail
        self.send_slice, self.recv_slice, o = {}, {}, 0
        for q in self.send_peers:
            self.send_slice[q] = (o, o + len(lp.send_ids[q]))
            o += len(lp.send_ids[q])
        for q in self.recv_peers:
            ids = np.asarray(lp.recv_ids[q], dtype=np.int64)
            if not np.array_equal(ids, np.arange(ids[0], ids[0] + ids.size)):
                raise ValueError(f"the ghosts owned by rank {q} are not contiguous in the local numbering")
            self.recv_slice[q] = (int(ids[0]) - lp.n_owned, int(ids[0]) - lp.n_owned + ids.size)
        self.bytes_per_exchange = 8 * self.nvar * self.n_send
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.host_staged = self.world > 1 and dist.get_backend(group) == "gloo"
        if self.host_staged:
            pin = self.dev.type == "cuda"
            mk = lambda rows: torch.empty((rows, self.nvar), dtype=torch.float64, pin_memory=pin)
            self.send_host, self.recv_host = mk(self.n_send), mk(self.n_ghost)
            self.vals_host = torch.empty(8, dtype=torch.float64, pin_memory=pin)
            if wide:
                self.wide_host = torch.empty(WIDE_MAX, dtype=torch.float64, pin_memory=pin)
        self.exchanges = self.allreduces = self.sized_exchanges = 0
        self.peers = peers
        self.peer_counts = (np.array([len(lp.send_ids.get(q, ())) for q in peers], dtype=np.int64),
                            np.array([len(lp.recv_ids.get(q, ())) for q in peers], dtype=np.int64))
        # the plan's send list and the ghost tail are grouped by peer in this order, or the counts would not describe them
        o = 0
        for q in peers:
            if q in self.recv_slice and self.recv_slice[q][0] != o:
                raise ValueError("the ghost tail is not grouped by owner in ascending rank order")
            o += len(lp.recv_ids.get(q, ()))
        self.error = None
        self._views, self._streams, self._pending, self._recv, self._recv_sized = {}, {}, [], None, None
        # the ctypes function objects must outlive every call that uses the struct
        self._cb = (EXCHANGE_BEGIN_FN(self._guard(self._c_begin)), EXCHANGE_END_FN(self._guard(self._c_end)),
                    ALLREDUCE_SUM_FN(self._guard(self._c_allreduce)))
        self.struct = SolveCommStruct(None, *self._cb)
        self.sized_struct = None
        if sized:
            self._cb_sized = (EXCHANGE_SIZED_BEGIN_FN(self._guard(self._c_sized_begin)), EXCHANGE_END_FN(self._guard(self._c_sized_end)))
            self.sized_struct = SolveCommSizedStruct(self.struct, *self._cb_sized)
        self.wide_struct, self.wide_allreduces, self.wide_lengths = None, 0, []
        if wide:
            self._cb_wide = ALLREDUCE_SUM_FN(self._guard(self._c_allreduce_wide))
            inner = self.sized_struct if sized else SolveCommSizedStruct(self.struct)   # no peers: the sized pair stays NULL
            self.wide_struct = SolveCommWideStruct(inner, self._cb_wide)

    # -- raw addresses -> torch
    def _view(self, addr, rows):
        """zero-copy [rows][nvar] view of device memory at addr (the library's send buffer, a vector's ghost tail, the record)"""
        if rows == 0 or not addr:
            return torch.empty((0, self.nvar), dtype=torch.float64, device=self.dev)
        key = (addr, rows)
        if key not in self._views:
            class _V:
                pass
            v = _V()
            v.__cuda_array_interface__ = {"shape": (rows, self.nvar), "typestr": "<f8", "data": (addr, False), "version": 2, "strides": None}
            self._views[key] = torch.as_tensor(v, device=self.dev)
        return self._views[key]

    def _stream(self, ptr):
        if not ptr:
            return torch.cuda.default_stream(self.dev)
        if ptr not in self._streams:
            self._streams[ptr] = torch.cuda.ExternalStream(ptr, device=self.dev)
        return self._streams[ptr]

    def _guard(self, f):
        def call(*a):
            try:
                return int(f(*a) or 0)
            except BaseException as e:   # must not propagate into the C caller
                self.error = e
                return 1
        return call

    def _c_begin(self, user, d_send, d_recv, stream):
        return self.begin(self._view(d_send, self.n_send), self._view(d_recv, self.n_ghost), self._stream(stream))

    def _c_end(self, user, stream):
        return self.end(self._stream(stream))

    def _c_allreduce(self, user, d_vals, n, stream):
        class _V:
            pass
        key = ("vals", d_vals)
        if key not in self._views:
            v = _V()
            v.__cuda_array_interface__ = {"shape": (8,), "typestr": "<f8", "data": (d_vals, False), "version": 2, "strides": None}
            self._views[key] = torch.as_tensor(v, device=self.dev)
        return self.allreduce(self._views[key][:n], self._stream(stream))

    def _c_allreduce_wide(self, user, d_vals, n, stream):
        if not 1 <= n <= WIDE_MAX:
            raise ValueError(f"the library asks for a wide all-reduce of {n} doubles, outside 1 .. {WIDE_MAX}")
        return self.allreduce_wide(self._flat(d_vals, WIDE_MAX)[:n], self._stream(stream))

    def _flat(self, addr, count):
        """zero-copy [count] view of device memory at addr"""
        if count == 0 or not addr:
            return torch.empty(0, dtype=torch.float64, device=self.dev)
        key = ("flat", addr, count)
        if key not in self._views:
            class _V:
                pass
            v = _V()
            v.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (addr, False), "version": 2, "strides": None}
            self._views[key] = torch.as_tensor(v, device=self.dev)
        return self._views[key]

    def _c_sized_begin(self, user, d_send, d_recv, n_peers, send_off, recv_off, stream):
        if n_peers != len(self.peers):
            raise ValueError(f"the library names {n_peers} peers, this communicator has {len(self.peers)}")
        so, ro = [int(send_off[k]) for k in range(n_peers + 1)], [int(recv_off[k]) for k in range(n_peers + 1)]
        return self.sized_begin(self._flat(d_send, so[-1]), self._flat(d_recv, ro[-1]), so, ro, self._stream(stream))

    def _c_sized_end(self, user, stream):
        return self.sized_end(self._stream(stream))

    # -- the sized exchange on tensors.  send / recv: flat, send_off[-1] and recv_off[-1] doubles; peer k of self.peers owns
    #    send[send_off[k]:send_off[k + 1]] and fills recv[recv_off[k]:recv_off[k + 1]]
    def sized_begin(self, send, recv, send_off, recv_off, stream):
        self.sized_exchanges += 1
        if self.world == 1 or not self.peers:
            return 0
        with torch.cuda.stream(stream):
            if self.host_staged:
                sb, rb = self.send_host.view(-1)[:send.numel()], self.recv_host.view(-1)[:recv.numel()]
                if send.numel():
                    sb.copy_(send, non_blocking=True)
                stream.synchronize()
                self._recv_sized = (recv, rb)
            else:
                sb, rb, self._recv_sized = send, recv, None
            ops = [dist.P2POp(dist.irecv, rb[recv_off[k]:recv_off[k + 1]], q, group=self.group)
                   for k, q in enumerate(self.peers) if recv_off[k + 1] > recv_off[k]]
            ops += [dist.P2POp(dist.isend, sb[send_off[k]:send_off[k + 1]], q, group=self.group)
                    for k, q in enumerate(self.peers) if send_off[k + 1] > send_off[k]]
            self._pending = dist.batch_isend_irecv(ops) if ops else []
        return 0

    def sized_end(self, stream):
        if self.world == 1 or not self.peers:
            return 0
        with torch.cuda.stream(stream):
            for w in self._pending:
                w.wait()
            self._pending = []
            if self._recv_sized is not None and self._recv_sized[0].numel():
                self._recv_sized[0].copy_(self._recv_sized[1], non_blocking=True)
        return 0

    # -- the three callbacks on tensors.  send: [n_send][nvar], packed; recv: [n_ghost][nvar], the ghost tail; stream: the library's
    def begin(self, send, recv, stream):
        self.exchanges += 1
        if self.world == 1 or not (self.send_peers or self.recv_peers):
            return 0
        with torch.cuda.stream(stream):
            if self.host_staged:
                if self.n_send:
                    self.send_host.copy_(send, non_blocking=True)
                stream.synchronize()
                sb, rb, self._recv = self.send_host, self.recv_host, recv
            else:
                sb, rb, self._recv = send, recv, None
            ops = [dist.P2POp(dist.irecv, rb[slice(*self.recv_slice[q])], q, group=self.group) for q in self.recv_peers]
            ops += [dist.P2POp(dist.isend, sb[slice(*self.send_slice[q])], q, group=self.group) for q in self.send_peers]
            self._pending = dist.batch_isend_irecv(ops)
        return 0

    def end(self, stream):
        if self.world == 1 or not (self.send_peers or self.recv_peers):
            return 0
        with torch.cuda.stream(stream):
            for w in self._pending:
                w.wait()
            self._pending = []
            if self._recv is not None and self.n_ghost:
                self._recv.copy_(self.recv_host, non_blocking=True)
        return 0

    def allreduce_wide(self, vals, stream):
        """vals: [n] device doubles, n <= 130, summed over the ranks in place"""
        self.wide_allreduces += 1
        self.wide_lengths.append(int(vals.numel()))
        if self.world == 1:
            return 0
        with torch.cuda.stream(stream):
            if self.host_staged:
                h = self.wide_host[:vals.numel()]
                h.copy_(vals, non_blocking=True)
                stream.synchronize()
                dist.all_reduce(h, group=self.group)
                vals.copy_(h, non_blocking=True)
            else:
                dist.all_reduce(vals, group=self.group)
        return 0

    def allreduce(self, vals, stream):
        self.allreduces += 1
        if self.world == 1:
            return 0
        with torch.cuda.stream(stream):
            if self.host_staged:
                h = self.vals_host[:vals.numel()]
                h.copy_(vals, non_blocking=True)
                stream.synchronize()
                dist.all_reduce(h, group=self.group)
                vals.copy_(h, non_blocking=True)
            else:
                dist.all_reduce(vals, group=self.group)
        return 0
