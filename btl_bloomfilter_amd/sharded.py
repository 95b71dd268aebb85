"""Hash-range sharded Bloom filter over the GPUs of one node.

One process per GPU (torch.distributed; backend "nccl" = RCCL over xGMI).  The M-bit filter is cut
into `world` contiguous bit ranges; rank g holds bits [g*M/W, (g+1)*M/W) in its HBM.  Probe
positions are `hash % M` exactly as in the single-GPU filter (BloomFilter.hpp:190), so the shard
bodies concatenated in rank order ARE the single-filter body (and the .bf file).

Three data paths:
  gather (default for 2..4 ranks; any geometry; bit and counting filters): reads move, probes do not.
    Every rank sends its reads to all peers (1 byte per base), hashes its own chunk while they travel
    and then the peers' chunks, and keeps the probes that fall into its own bit range (pass A's WINDOW
    variant; passes B and C then see the shard's 1/W of the probes).  A query answers "every probe of
    this window inside my range is set" per shard; the partial bitmaps go back to the reads' owners
    and are ANDed.  W times the hashing for 1/8 (W = 2) to 1/12 (W = 4) of the traffic: xGMI is one link per GPU
    pair, so the probe exchange below is link-bound at small W.
  routed (8 ranks; power-of-two geometries, large batches): the global position space is cut into
    512 bins; each rank hashes its reads and radix-partitions the probe positions into those bins in
    LDS (4-byte entries, 128-byte chunks); the block of bins a shard owns is contiguous, so ONE
    fixed-size all-to-all moves it; the owner splits the received bins down to 64 KiB segments and
    ORs / tests them in LDS.  A query sends nothing back but the few positions found clear
    (all-gather of small fail lists); the origin clears the windows that own one of them.
  direct (any geometry; the stand-in ops of the CPU tests):
    insert : every rank buckets the h positions of each k-mer by owning shard; ONE all-to-all moves
             shard-local positions to their owners; owners atomicOr them into their bit range.
    query  : all-to-all of positions out, owners test bits, all-to-all of one byte per probe back in
             the same order; the origin ANDs the h answers of each k-mer into the per-window bitmap.

The exchange (of reads or of probes) is the only collective on the data path and it is a real data
dependency: the h probes of one k-mer land on different shards.  Work is cut into batches of reads so
that buffer memory stays bounded.

`ops` abstracts the per-rank compute: HipShardOps (the C ABI / HIP kernels) in production; the
tests substitute a CPU stand-in to exercise this routing logic under gloo with world_size 2.
_Transport is the only code that talks to the process group."""
import ctypes as C
import math
import os
from dataclasses import dataclass

import torch
import torch.distributed as dist

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class HipShardOps:
    """per-rank compute through the C ABI (HIP kernels); tensors live on cuda:<device>"""

    def __init__(self, global_bits, hash_num, kmer_size, rank, world, device, counting=False, threshold=0):
        """global_bits: bits of the whole filter, or its uint8_t counters when counting"""
        self.L = _lib.load()
        self.h = hash_num
        self.k = kmer_size
        self.world = world
        self.counting = bool(counting)
        self.device_index = device
        self.device = torch.device("cuda", device)
        hnd = C.c_void_p()
        _lib.check(self.L.btlbf_create_shard(C.byref(hnd), _lib.COUNTING8 if counting else _lib.BLOOM, global_bits,
                                             rank, world, hash_num, kmer_size, threshold, device))
        self.f = hnd
        # owner scratch the routed passes so far have made this filter allocate, as the batch planner remembers it
        # (asking the library instead needs a new ABI call: ADVICE.md)
        self.owner_scratch_held = 0

    def close(self):
        if self.f:
            self.L.btlbf_destroy(self.f)
            self.f = None

    def _sp(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _lay(self, read_len):
        lay = _lib.Layout()
        lay.starts, lay.n_seqs, lay.read_len = None, 0, read_len
        return lay

    def clear(self):
        _lib.check(self.L.btlbf_clear(self.f, self._sp()))

    def positions(self, reads, read_len, cap, want_tags):
        n = reads.numel()
        buckets = torch.empty((self.world, cap), dtype=torch.int64, device=self.device)
        tags = torch.empty((self.world, cap), dtype=torch.int64, device=self.device) if want_tags else None
        counts = torch.zeros(self.world, dtype=torch.int64, device=self.device)
        valid = torch.zeros((n + 63) // 64, dtype=torch.int64, device=self.device) if want_tags else None
        _lib.check(self.L.btlbf_positions_seqs(self.f, _ptr(reads), n, C.byref(self._lay(read_len)), self.world,
                                               _ptr(buckets), _ptr(tags), cap, _ptr(counts), _ptr(valid), self._sp()))
        return buckets, tags, counts, valid

    def insert_positions(self, pos):
        _lib.check(self.L.btlbf_insert_positions(self.f, _ptr(pos), pos.numel(), self._sp()))

    def test_positions(self, pos):
        out = torch.empty(pos.numel(), dtype=torch.uint8, device=self.device)
        _lib.check(self.L.btlbf_test_positions(self.f, _ptr(pos), pos.numel(), _ptr(out), self._sp()))
        return out

    def and_answers(self, tags, answers, hit_bits):
        _lib.check(self.L.btlbf_and_answers(_ptr(tags), _ptr(answers), tags.numel(), self.h, _ptr(hit_bits),
                                            self.device_index, self._sp()))

    def popcount_bits(self, bits):
        n = bits.numel() * bits.element_size()
        pad = (-n) % 16
        if pad:
            bits = torch.cat([bits.view(torch.uint8), torch.zeros(pad, dtype=torch.uint8, device=bits.device)])
            n += pad
        out = C.c_uint64()
        _lib.check(self.L.btlbf_popcount_bits(_ptr(bits), n, C.byref(out), self.device_index, self._sp()))
        return out.value

    # ---- gather mode: the shard is handed every rank's reads and keeps the probes inside its window ----
    def insert_seqs(self, reads, read_len):
        _lib.check(self.L.btlbf_insert_seqs(self.f, _ptr(reads), reads.numel(), C.byref(self._lay(read_len)),
                                            _lib.INCREMENT_ALL, _lib.ORDER_PARALLEL, _lib.DEVICE, self._sp()))

    def contains_seqs(self, reads, read_len, hit_bits, valid_bits):
        """hit bit p = window p is clean and every probe of it that falls into this shard is set"""
        _lib.check(self.L.btlbf_contains_seqs(self.f, _ptr(reads), reads.numel(), C.byref(self._lay(read_len)),
                                              _ptr(hit_bits), _ptr(valid_bits), None, _lib.DEVICE, self._sp()))

    # ---- routing on the partitioned pipeline (btlbf_route_* / btlbf_apply_routed) ----
    def _route_windows(self, world):
        nw, spw = C.c_uint(), C.c_uint()
        return self.L.btlbf_route_windows(self.f, world, C.byref(nw), C.byref(spw)), (nw.value, spw.value)

    def route_supported(self, global_bits, world):
        """power-of-two geometry of at least 512 bins x one 64 KiB segment; filters above 2^42 positions are
        routed in windows of 2^42 and need at least one shard per window (btlbf_route_windows)"""
        pow2 = lambda x: x > 0 and (x & (x - 1)) == 0  # noqa: E731
        if not (pow2(global_bits) and pow2(world) and 1 <= self.h <= 8):
            return False
        return self._route_windows(world)[0] == _lib.OK

    def route_windows(self):
        """(position windows, shards per window): window w is owned by shards [w * spw, (w + 1) * spw)"""
        rc, windows = self._route_windows(self.world)
        _lib.check(rc)
        return windows

    def route_plan(self, plan_len, read_len):
        e, c = C.c_uint64(), C.c_uint64()
        _lib.check(self.L.btlbf_route_plan(self.f, plan_len, C.byref(self._lay(read_len)), self.world, C.byref(e),
                                           C.byref(c)))
        return e.value, c.value

    def route(self, reads, read_len, plan_len, query, send_ent, send_cnt, hit, valid, counts, spill, spill_count,
              window=0):
        _lib.check(self.L.btlbf_route_seqs(self.f, _ptr(reads), reads.numel(), C.byref(self._lay(read_len)), plan_len,
                                           self.world, int(window), int(query), _ptr(send_ent), _ptr(send_cnt),
                                           _ptr(hit), _ptr(valid), _ptr(counts), _ptr(spill), spill.numel(),
                                           _ptr(spill_count), self._sp()))

    def apply_routed(self, recv_ent, recv_cnt, n_blocks, plan_len, read_len, query, fail_list, fail_count):
        _lib.check(self.L.btlbf_apply_routed(self.f, _ptr(recv_ent), _ptr(recv_cnt), n_blocks, plan_len,
                                             C.byref(self._lay(read_len)), self.world, int(query), _ptr(fail_list),
                                             fail_list.numel() if fail_list is not None else 0, _ptr(fail_count),
                                             self._sp()))

    def route_geometry(self, plan_len, read_len):
        """(level-0 bins per shard, regions per bin, 128-byte chunks per region, bins per group)"""
        out = (C.c_uint32 * 4)()
        _lib.check(self.L.btlbf_route_geometry(self.f, plan_len, C.byref(self._lay(read_len)), self.world, self.world,
                                               out))
        return tuple(int(v) for v in out)

    def owner_scratch_bytes(self, plan_len, read_len):
        """bytes of scratch apply_routed[_bins] allocates inside the filter for batches of plan_len bytes of reads"""
        out = C.c_uint64()
        _lib.check(self.L.btlbf_owner_scratch_bytes(self.f, plan_len, C.byref(self._lay(read_len)), self.world,
                                                    self.world, C.byref(out)))
        return out.value

    def apply_routed_bins(self, recv_ent, recv_cnt, n_blocks, first_bin, n_bins, plan_len, read_len, query, fail_list,
                          fail_count):
        _lib.check(self.L.btlbf_apply_routed_bins(self.f, _ptr(recv_ent), _ptr(recv_cnt), n_blocks, first_bin, n_bins,
                                                  plan_len, C.byref(self._lay(read_len)), self.world, int(query),
                                                  _ptr(fail_list), fail_list.numel() if fail_list is not None else 0,
                                                  _ptr(fail_count), self._sp()))

    def apply_spill(self, pos, query, fail_list, fail_count):
        _lib.check(self.L.btlbf_apply_spill(self.f, _ptr(pos), pos.numel(), int(query), _ptr(fail_list),
                                            fail_list.numel() if fail_list is not None else 0, _ptr(fail_count),
                                            self._sp()))

    def resolve(self, reads, read_len, fails, hit_bits):
        _lib.check(self.L.btlbf_resolve_seqs(self.f, _ptr(reads), reads.numel(), C.byref(self._lay(read_len)),
                                             _ptr(fails), fails.numel(), _ptr(hit_bits), self._sp()))

    def local_body(self):
        import numpy as np

        n = self.L.btlbf_local_bytes(self.f)
        out = np.zeros(n, np.uint8)
        _lib.check(self.L.btlbf_download(self.f, C.c_void_p(out.ctypes.data), 0, n))
        return out

    def store_shard(self, path):
        _lib.check(self.L.btlbf_store_shard(self.f, str(path).encode()))


class _Transport:
    """The process group and every collective the passes issue on it.  Two rules live here and nowhere else:
    no message is larger than MSG_BYTES, and with RCCL the piece a rank keeps for itself is a device copy, not
    a message.  gloo (the tests) moves host memory, so there device tensors are staged through the CPU."""

    # No single point-to-point message is larger than this.  Measured on this stack (ROCm 7.2 RCCL,
    # examples/sharded_rccl.cpp): a grouped ncclSend/ncclRecv of more than about 1 GiB delivered only
    # half of its bytes (973 MB arrives whole, 2.0 GB and 4.2 GB arrive halved), so large blocks are
    # exchanged as a sequence of grouped all-to-alls over slices.
    MSG_BYTES = 256 << 20

    def __init__(self, group):
        up = dist.is_initialized()
        self.group = group
        self.rank = dist.get_rank(group) if up else 0
        self.world = dist.get_world_size(group) if up else 1
        self.device = None  # of the per-rank compute: set by the owner once it has its ops
        # BTLBF_FORCE_EXCHANGE=1: run the routed path's exchange even with a single rank (a one-rank RCCL
        # group sends every block to itself) -- lets a one-GPU box exercise the real collective calls
        self.force_exchange = bool(os.environ.get("BTLBF_FORCE_EXCHANGE")) and up
        # "2": as in production the rank's own block bypasses the collective (which then carries only
        # zero-length messages in a one-rank group); "1": the own block goes through RCCL too
        self.self_through_rccl = os.environ.get("BTLBF_FORCE_EXCHANGE") == "1"
        # gloo moves host memory: stage device tensors through the CPU (test mode only)
        self.stage_cpu = (dist.get_backend(group) if up else "none") == "gloo"
        self.own_is_copy = not self.stage_cpu and not self.self_through_rccl

    def _grouped(self, outs, ins, async_op):
        """ONE all-to-all: ins[p] goes to rank p, outs[p] comes from it (1-D slices, empty ones included).
        Returns the work handle, or None when there is nothing to wait for"""
        if not self.stage_cpu:
            return dist.all_to_all(outs, ins, group=self.group, async_op=async_op)
        # gloo: the single-tensor form on packed host copies of the slices
        sizes = [o.numel() for o in outs]
        tmp = torch.empty(sum(sizes), dtype=ins[0].dtype)
        dist.all_to_all_single(tmp, torch.cat(ins).cpu(), output_split_sizes=sizes,
                               input_split_sizes=[i.numel() for i in ins], group=self.group)
        for o, part in zip(outs, tmp.split(sizes)):
            o.copy_(part)
        return None

    def _step(self, t):
        return max(1, self.MSG_BYTES // t.element_size())

    def _sliced(self, outs, ins, longest, async_op=False):
        """_grouped over slices of at most MSG_BYTES of messages of up to `longest` elements (every rank passes
        the same `longest`; a message that has run out contributes empty slices) -> the work handles"""
        step = self._step(ins[0])
        works = [self._grouped([o[c: c + step] for o in outs], [i[c: c + step] for i in ins], async_op)
                 for c in range(0, longest, step)]
        return [w for w in works if w is not None]

    def max(self, v):
        if self.world == 1:
            return int(v)
        t = torch.tensor([int(v)], dtype=torch.int64)
        if not self.stage_cpu:
            t = t.to(self.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return int(t.item())

    def exchange_counts(self, counts):
        """counts[p] = what this rank has for rank p -> what rank p has for this rank"""
        if self.world == 1:
            return counts
        c = counts.cpu() if self.stage_cpu else counts
        out = torch.empty_like(c)
        dist.all_to_all_single(out, c, group=self.group)
        return out

    def all_to_all(self, send, send_counts, recv_counts):
        """variable-size all-to-all of a flat tensor; counts are python ints per peer"""
        if self.world == 1:
            return send
        recv = torch.empty(sum(recv_counts), dtype=send.dtype, device=send.device)
        step = self._step(send)
        rounds = self.max(-(-max(max(send_counts), max(recv_counts), 1) // step))
        if rounds <= 1 and not self.stage_cpu:
            dist.all_to_all_single(recv, send, output_split_sizes=recv_counts, input_split_sizes=send_counts,
                                   group=self.group)
        else:
            self._sliced(recv.split(recv_counts), send.split(send_counts), rounds * step)
        return recv

    def rows_all_to_all(self, r2, s2, async_op, first=0, receiving=True):
        """row i of s2 goes to rank first + i (s2 has one row per TARGET rank: all ranks, or the owners of
        one position window), row p of r2 comes from rank p when this rank is `receiving` (2-D tensors whose
        rows are contiguous; the rows of s2 may be slices of larger blocks).  At most MSG_BYTES per message;
        returns the work handles.  With RCCL the row a rank keeps for itself does not go through the
        collective at all: it is one device-to-device copy on the compute stream (BTLBF_FORCE_EXCHANGE=1
        keeps it in, for tests)."""
        W, per = self.world, s2.shape[1]
        targets = range(first, first + s2.shape[0])
        if len(targets) == W and receiving and per <= self._step(s2) and not self.own_is_copy and not self.stage_cpu \
                and s2.is_contiguous() and r2.is_contiguous():
            return [dist.all_to_all_single(r2.view(-1), s2.view(-1), group=self.group, async_op=async_op)]
        wire = lambda p: not (self.own_is_copy and p == self.rank)  # noqa: E731
        works = self._sliced([r2[p] if receiving and wire(p) else r2[p, :0] for p in range(W)],
                             [s2[p - first] if p in targets and wire(p) else s2[0, :0] for p in range(W)],
                             per, async_op)
        if self.own_is_copy and receiving and self.rank in targets:
            r2[self.rank].copy_(s2[self.rank - first])
        return works

    def gather(self, out, piece, peers):
        """out[i] := the piece of rank peers[i], in messages of at most MSG_BYTES, asynchronous (returns the
        work handles).  A rank is its own peer only in the one-rank test modes (BTLBF_FORCE_EXCHANGE): its
        piece then goes through RCCL ("1") or is a device copy ("2")."""
        W, n = self.world, piece.numel()
        if not peers:
            return []
        o2 = out.view(len(peers), n)
        idx = {p: i for i, p in enumerate(peers)}
        if self.stage_cpu:  # gloo has an all-gather of host tensors, and the tests have always used it here
            parts = [torch.empty(n, dtype=piece.dtype) for _ in range(W)]
            dist.all_gather(parts, piece.cpu(), group=self.group)
            for p in peers:
                o2[idx[p]].copy_(parts[p])
            return []
        none = piece[:0]
        local = self.own_is_copy and self.rank in idx
        wire = lambda p: p in idx and not (p == self.rank and local)  # noqa: E731  (p's piece arrives over RCCL)
        works = self._sliced([o2[idx[p]] if wire(p) else none for p in range(W)],
                             [piece if (p != self.rank or wire(p)) else none for p in range(W)], n, async_op=True)
        if local:
            o2[idx[self.rank]].copy_(piece)
        return works

    def all_gather_var(self, t, n):
        """all-gather the first n elements of the 1-D int64 tensor t from every rank -> 1-D tensor"""
        if self.world == 1:
            return t[:n]
        dev = t.device
        wire_dev = "cpu" if self.stage_cpu else dev
        cnt = torch.tensor([n], dtype=torch.int64, device=wire_dev)
        cnts = [torch.zeros_like(cnt) for _ in range(self.world)]
        dist.all_gather(cnts, cnt, group=self.group)
        cnts = [int(c.item()) for c in cnts]
        m = max(cnts)
        if m == 0:
            return t[:0]
        pad = torch.zeros(m, dtype=t.dtype, device=wire_dev)
        pad[:n] = t[:n].to(pad.device)
        outs = [torch.empty_like(pad) for _ in range(self.world)]
        dist.all_gather(outs, pad, group=self.group)
        return torch.cat([o[:c] for o, c in zip(outs, cnts)]).to(dev)


@dataclass(frozen=True)
class _RouteShape:
    """what fixes the buffers and the schedule of a routed pass, whatever the batch size"""
    W: int             # ranks
    n_win: int         # position windows; every batch is routed once per window
    spw: int           # shards per window: window w is owned by ranks [w * spw, (w + 1) * spw)
    my_win: int        # the window this rank owns a part of
    G: int             # groups the level-0 bins of a shard travel and are applied in (1 without an exchange)
    gb: int            # bins per group
    n_slots: int       # send block sets: two when the next job is routed while this one is exchanged
    r_slots: int       # receive buffers of one group each
    exchanging: bool   # there are peers (or BTLBF_FORCE_EXCHANGE)
    pipelined: bool


class _RoutedPass:
    """The buffers, streams and events of one routed pass, and what is done to a JOB = (batch of reads, position
    window): route it into a send block set, collect what spilled, exchange and apply its groups."""

    def __init__(self, f, shape, reads, read_len, query, hit_bits, batch):
        s, ops, dev = shape, f.ops, f.ops.device
        self.f, self.ops, self.net, self.s = f, ops, f.net, shape
        self.reads, self.read_len, self.query, self.hit_bits, self.batch = reads, read_len, query, hit_bits, batch
        self.ent_b, self.cnt_b = ops.route_plan(batch, read_len)
        self.ge, self.gc = self.ent_b // s.G, self.cnt_b // s.G  # bytes of one group inside one block
        assert self.ge * s.G == self.ent_b and self.gc * s.G == self.cnt_b and self.ge % 8 == 0
        self.send_ent = [torch.empty(s.spw * self.ent_b, dtype=torch.uint8, device=dev) for _ in range(s.n_slots)]
        self.send_cnt = [torch.empty(s.spw * self.cnt_b, dtype=torch.uint8, device=dev) for _ in range(s.n_slots)]
        if s.exchanging:
            self.recv_ent = [torch.empty(s.W * self.ge, dtype=torch.uint8, device=dev) for _ in range(s.r_slots)]
            self.recv_cnt = [torch.empty(s.W * self.gc, dtype=torch.uint8, device=dev) for _ in range(s.r_slots)]
        self.spill = [torch.empty(f.SPILL_CAP, dtype=torch.int64, device=dev) for _ in range(s.n_slots)]
        self.spill_count = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(s.n_slots)]
        # the host learns a job's spill count from a pinned copy made on the ROUTING stream right behind the routing
        # (a .item() on the caller's stream would wait for the exchange and apply work queued there)
        self.spill_host = [torch.zeros(1, dtype=torch.int64).pin_memory() if dev.type == "cuda" else None
                           for _ in range(s.n_slots)]
        self.spilled = []  # explicit positions of the jobs done so far (device tensors)
        self.fail = torch.empty(f.FAIL_CAP, dtype=torch.int64, device=dev) if query else None
        self.fail_count = torch.zeros(1, dtype=torch.int64, device=dev) if query else None
        self.cnt2 = torch.zeros(2, dtype=torch.int64, device=dev) if query else None
        # pipelined: routing runs on its own stream, the exchange + apply of the previous job on the caller's
        self.cur = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
        self.side = torch.cuda.Stream(dev) if (s.pipelined and self.cur is not None) else None
        self.routed_ev, self.free_ev = [None] * s.n_slots, [None] * s.n_slots
        if self.side is not None:
            self.side.wait_stream(self.cur)

    def _do_route(self, j, slot, again=False):
        bi, w = divmod(j, self.s.n_win)
        off = bi * self.batch
        chunk = self.reads[off: off + self.batch]  # empty once this rank has run out of reads: it still takes part
        view = None
        if self.query:
            w0, nw = off // 64, (chunk.numel() + 63) // 64
            view = self.hit_bits[w0: w0 + nw]
        self.spill_count[slot].zero_()
        # every window's pass re-initialises the hit bits of the batch (hit = valid; failures are resolved at the end
        # of the pass) but the clean windows are counted once (a job routed a second time has already counted its own)
        self.ops.route(chunk, self.read_len, self.batch, self.query, self.send_ent[slot], self.send_cnt[slot], view,
                       None, self.cnt2 if w == 0 and not again else None, self.spill[slot], self.spill_count[slot],
                       window=w)

    # NOTE for the C ABI: ops.route (btlbf_route_seqs) must stay free of per-filter scratch -- it runs on a second
    # stream while btlbf_apply_routed* uses the filter's scratch on the first (host_partition.cpp: route passes no late list,
    # so pass A takes its plain schedule there; tests/test_sharded.py runs both streams together)
    def route(self, j):
        slot = j % self.s.n_slots
        if self.side is None:
            self._do_route(j, slot)
            return
        if self.free_ev[slot] is not None:
            self.side.wait_event(self.free_ev[slot])  # the exchanges that read this block set have completed
        with torch.cuda.stream(self.side):
            self._do_route(j, slot)
            self.spill_host[slot].copy_(self.spill_count[slot], non_blocking=True)
            self.routed_ev[slot] = torch.cuda.Event()
            self.routed_ev[slot].record(self.side)

    def collect_spill(self, j, slot):
        """the job's explicit positions; a list that overflowed (heavily skewed input: poly-A reads, one
        read a million times) is routed again into one that is large enough -- nothing of the job has
        left this rank yet"""
        if self.routed_ev[slot] is not None:
            self.routed_ev[slot].synchronize()  # the job's routing (and the copy of its count): nothing else
            n = int(self.spill_host[slot][0])
        else:
            n = int(self.spill_count[slot].item())
        while n > self.spill[slot].numel():
            self.spill[slot] = torch.empty(n + n // 4 + 1024, dtype=torch.int64, device=self.ops.device)
            self._do_route(j, slot, again=True)  # on the caller's stream; the blocks come out equivalent
            n = int(self.spill_count[slot].item())
        if n:
            self.spilled.append(self.spill[slot][:n].clone())

    def exchange(self, slot, g, w):
        """start the exchange of group g of the job in `slot` into receive buffer g % r_slots -> work handles"""
        s, rs, works = self.s, g % self.s.r_slots, []
        for snd, rcv, per_block, gbytes in ((self.send_ent[slot], self.recv_ent[rs], self.ent_b, self.ge),
                                            (self.send_cnt[slot], self.recv_cnt[rs], self.cnt_b, self.gc)):
            # rows [spw, group bytes] of group g inside the blocks of the send set, as 8-byte elements if possible
            # (keeps per-peer element counts far below 2^31)
            if gbytes % 8 == 0 and per_block % 8 == 0:
                s2 = snd.view(torch.int64).view(s.spw, per_block // 8)[:, g * gbytes // 8: (g + 1) * gbytes // 8]
                r2 = rcv.view(torch.int64).view(s.W, gbytes // 8)
            else:
                s2 = snd.view(s.spw, per_block)[:, g * gbytes: (g + 1) * gbytes]
                r2 = rcv.view(s.W, gbytes)
            works += self.net.rows_all_to_all(r2, s2, async_op=not self.net.stage_cpu, first=w * s.spw,
                                              receiving=(w == s.my_win))
        return works

    def finish(self, j):
        s, ops = self.s, self.ops
        slot, w = j % s.n_slots, j % s.n_win
        self.collect_spill(j, slot)
        if self.side is not None:
            self.cur.wait_event(self.routed_ev[slot])
        if not s.exchanging:
            ops.apply_routed(self.send_ent[slot], self.send_cnt[slot], s.W, self.batch, self.read_len, self.query,
                             self.fail, self.fail_count)
            return
        inflight = {g: self.exchange(slot, g, w) for g in range(min(s.r_slots, s.G))}
        for g in range(s.G):
            for x in inflight.pop(g):
                x.wait()  # RCCL: the compute stream waits, the host does not
            rs = g % s.r_slots
            if w == s.my_win:
                ops.apply_routed_bins(self.recv_ent[rs], self.recv_cnt[rs], s.W, g * s.gb, s.gb, self.batch,
                                      self.read_len, self.query, self.fail, self.fail_count)
            if g + s.r_slots < s.G:
                inflight[g + s.r_slots] = self.exchange(slot, g + s.r_slots, w)  # into the buffer just applied
        if self.side is not None:
            self.free_ev[slot] = torch.cuda.Event()
            self.free_ev[slot].record(self.cur)

    def epilogue(self, counts):
        """after the last job: the spilled positions of all ranks, and for a query the fail lists -> False when
        there are more failed probes than the lists hold"""
        f, ops, net, reads = self.f, self.ops, self.net, self.reads
        if self.side is not None:
            self.cur.wait_stream(self.side)
        # entries that could not be staged at their origin travel as explicit positions (rare)
        mine = torch.cat(self.spilled) if self.spilled else torch.empty(0, dtype=torch.int64, device=ops.device)
        gathered = net.all_gather_var(mine, mine.numel())
        if gathered.numel():
            ops.apply_spill(gathered, self.query, self.fail, self.fail_count)
        if self.query:
            n_fail = int(self.fail_count.item())
            if net.max(1 if n_fail > f.FAIL_CAP else 0):
                return False  # miss-heavy: the caller redoes the query on the direct path
            fails = net.all_gather_var(self.fail, n_fail)
            if fails.numel() > f.FAIL_CAP:
                return False
            if fails.numel() and reads.numel():
                ops.resolve(reads, self.read_len, fails, self.hit_bits)
            f._fill_counts(counts, self.cnt2[0], reads, self.hit_bits)
        return True


class ShardedBloomFilter:
    """counting=True: a sharded CountingBloomFilter<uint8_t> of `global_bits` counters -- insert_reads is
    incrementAll (exact, saturating; shard-local at the owners) and contains_reads is
    "minimum >= threshold"; gather mode or the routed path (the conservative update needs the h counters
    of a k-mer, which live on different shards, and is not offered)."""

    def __init__(self, global_bits, hash_num, kmer_size, device=0, group=None, ops=None, batch_reads=2_000_000,
                 slack=1.25, route=True, batch_bytes_cap=0, pipeline=None, counting=False, threshold=0, mode=None):
        self.net = _Transport(group)
        self.rank, self.world = self.net.rank, self.net.world
        if global_bits % (64 * self.world):
            raise ValueError("filter bits must split into multiples of 64 per shard")
        self.bits = global_bits
        self.h = hash_num
        self.k = kmer_size
        self.counting = bool(counting)
        self.ops = ops if ops is not None else HipShardOps(global_bits, hash_num, kmer_size, self.rank, self.world,
                                                           device, counting=counting, threshold=threshold)
        self.net.device = self.ops.device
        self.batch_reads = batch_reads
        self.slack = slack
        self.route_enabled = route         # use the partitioned routing path when the geometry allows
        # "gather": every rank receives every rank's reads (1 byte per base over xGMI instead of 4 bytes
        # per probe) and applies the probes inside its own window -- W times the hashing, no probe
        # exchange; "exchange": the routed / direct paths below.  auto = gather for 2..4 ranks: xGMI is one
        # link per GPU pair, so the probe exchange is link-bound at small W.
        # "routed" / "direct" pin the exchange flavour: "routed" raises here when the geometry has no routed
        # path instead of quietly falling back to the (much slower) direct position exchange
        mode = mode or os.environ.get("BTLBF_SHARD_MODE") or "auto"
        if mode not in ("auto", "gather", "exchange", "routed", "direct"):
            raise ValueError("mode must be auto, gather, exchange, routed or direct")
        can_gather = hasattr(self.ops, "insert_seqs")
        if mode == "gather" and not can_gather:
            raise ValueError("gather mode: these ops have no whole-buffer insert")
        if mode == "direct":
            self.route_enabled = False
        if mode == "routed" and not self._routed():
            raise ValueError("routed mode: no routed path for a 2^%.1f-position filter on %d shards with these ops "
                             "(needs powers of two, at least 2^29 bits, h <= 8)"
                             % (math.log2(global_bits), self.world))
        self.mode = "gather" if can_gather and (mode == "gather" or (mode == "auto" and 2 <= self.world <= 4)) \
            else "exchange"
        if self.counting and self.mode != "gather" and not (route and self.ops.route_supported(global_bits, self.world)):
            raise ValueError("sharded counting filters need gather mode or the routed path (power-of-two "
                             "geometry, h <= 8)")
        self.batch_bytes_cap = batch_bytes_cap
        # routed path: keep the exchange of batch i in flight while batch i+1 is routed (two buffer
        # sets).  None = whenever the exchange is asynchronous (RCCL); True forces the same schedule
        # over a synchronous exchange (tests).
        self.pipeline = pipeline

    # the largest message of the exchange (see _Transport.MSG_BYTES); tests lower it on the instance
    MSG_BYTES = property(lambda self: self.net.MSG_BYTES, lambda self, v: setattr(self.net, "MSG_BYTES", v))

    def clear(self):
        self.ops.clear()

    def _fill_counts(self, counts, n_valid, reads, hit_bits):
        """the counts of a query pass: {clean windows, windows found = set bits of the pass's hit bitmap}"""
        if counts is not None:
            counts[0] = int(n_valid)
            counts[1] = self.ops.popcount_bits(hit_bits[: (reads.numel() + 63) // 64]) if reads.numel() else 0

    # ---- direct path: explicit positions to their owners, one byte per probe back ----------------
    def _bucketed(self, reads, read_len, want_tags):
        n_kmers = (reads.numel() // read_len) * max(read_len - self.k + 1, 0)
        cap = int(n_kmers * self.h / self.world * self.slack) + 4096
        if reads.numel() == 0:  # a rank that has run out of reads still takes part in the exchange
            dev = self.ops.device
            z = torch.zeros(self.world, dtype=torch.int64, device=dev)
            e = torch.empty(0, dtype=torch.int64, device=dev)
            recv_cnt = self.net.exchange_counts(z).cpu().tolist()
            return e, (e if want_tags else None), [0] * self.world, recv_cnt, \
                (torch.empty(0, dtype=torch.int64, device=dev) if want_tags else None)
        while True:
            buckets, tags, counts, valid = self.ops.positions(reads, read_len, cap, want_tags)
            cnt = counts.cpu().tolist()  # split sizes must be host integers
            if max(cnt) <= cap:
                break
            cap = max(cnt) + 4096  # skewed batch: retry once with the exact capacity
        send = torch.cat([buckets[s, : cnt[s]] for s in range(self.world)])
        stags = torch.cat([tags[s, : cnt[s]] for s in range(self.world)]) if want_tags else None
        recv_cnt = self.net.exchange_counts(counts).cpu().tolist()
        return send, stags, cnt, recv_cnt, valid

    def _batches(self, reads, read_len):
        """(offset, chunk) pairs; every rank runs the SAME number of iterations -- each one issues collectives --
        with empty chunks once its own reads are exhausted"""
        step = self.batch_reads * read_len
        n = self.net.max(-(-reads.numel() // step))
        for i in range(n):
            yield i * step, reads[i * step: (i + 1) * step]

    # ---- routed path: 4-byte partitioned entries, fixed-size all-to-all, owners apply in LDS ----
    FAIL_CAP = 4 << 20   # failed positions one owner may report per batch (library limit for resolve)
    SPILL_CAP = 1 << 20

    def _routed(self):
        return (self.route_enabled and hasattr(self.ops, "route_supported")
                and self.ops.route_supported(self.bits, self.world))

    def _route_shape(self, read_len):
        ops, W, net = self.ops, self.world, self.net
        exchanging = W > 1 or net.force_exchange
        pipelined = exchanging and (not net.stage_cpu if self.pipeline is None else bool(self.pipeline))
        n_win, spw = ops.route_windows() if hasattr(ops, "route_windows") else (1, W)
        bins, _, _, gb = ops.route_geometry(64 * read_len, read_len)  # per shard and per group: the same for any length
        G = bins // gb if exchanging else 1
        return _RouteShape(W=W, n_win=n_win, spw=spw, my_win=self.rank // spw, G=G, gb=gb,
                           n_slots=2 if pipelined else 1, r_slots=2 if G > 1 else 1, exchanging=exchanging,
                           pipelined=pipelined)

    def _route_batches(self, reads, read_len, shape):
        """(bytes of read buffer per batch, batches per pass), the same on every rank: the send block sets, the
        receive groups and the owner's split levels of a batch must fit in free HBM"""
        longest = self.net.max(reads.numel())
        if longest == 0:
            return 0, 0
        if self.ops.device.type == "cuda":
            # what the driver reports as free, plus what torch's caching allocator holds without using it
            # (the block sets of the previous pass): otherwise every pass after the first plans tiny batches
            free = torch.cuda.mem_get_info(self.ops.device)[0]
            free += torch.cuda.memory_reserved(self.ops.device) - torch.cuda.memory_allocated(self.ops.device)
        else:
            free = 1 << 40
        free = -self.net.max(-free)  # the smallest over ranks: every rank must plan the same batch
        exact = hasattr(self.ops, "owner_scratch_bytes") and not self.batch_bytes_cap
        plan = self._plan_exact(shape, longest, free, read_len) if exact else None
        return plan or self._plan_by_rule(shape, longest, free, read_len)

    def _plan_exact(self, s, longest, free, read_len):
        """the buffers of a pass added up exactly (send block sets, receive groups, the owner's scratch inside the
        filter, spill and fail lists), for the fewest batches that leave a tenth of the free HBM untouched: the
        rule of thumb keeps a fifth and more, which at BASELINE config 4 (128 GiB shards) is the difference
        between five batches per pass and four -- one sweep of the shard per pass.  None: not within 4096 batches"""
        unit = 64 * read_len
        lists = s.n_slots * self.SPILL_CAP * 8 + self.FAIL_CAP * 8 + (64 << 20)
        # (the owner's scratch of an earlier pass is still allocated inside the filter -- it only grows -- and will
        # be used again: it is not free, but it is not an additional need either)
        held = self.ops.owner_scratch_held
        for n_b in range(1, 4097):
            batch = -(-(-(-longest // n_b)) // unit) * unit
            ent_b, cnt_b = self.ops.route_plan(batch, read_len)
            owner = self.ops.owner_scratch_bytes(batch, read_len)
            total = s.n_slots * s.spw * (ent_b + cnt_b) + lists + max(owner - held, 0)
            if s.exchanging:
                total += s.r_slots * s.W * (ent_b // s.G + cnt_b // s.G)
            if total <= 0.90 * free or batch <= unit:
                self.ops.owner_scratch_held = max(held, owner)
                return batch, -(-longest // batch)
        return None

    def _plan_by_rule(self, s, longest, free, read_len):
        """per read byte: h*(L-k+1)/L probes * 4 B per entry, ~1.1x capacity; block sets: send, receive (when
        there are peers: two groups of a block set) + the owner's split levels, which hold 1/8 of a batch"""
        sets = s.n_slots / s.n_win + (s.r_slots / s.G if s.exchanging else 0.0) + 0.4
        per_byte = self.h * max(read_len - self.k + 1, 1) / read_len * 4 * 1.1 * sets
        unit = 64 * read_len
        batch = int(0.78 * free / per_byte) // unit * unit
        batch = max(batch, unit)
        if self.batch_bytes_cap:
            batch = min(batch, self.batch_bytes_cap // unit * unit or unit)
        n_batches = -(-longest // batch)
        batch = -(-(-(-longest // n_batches)) // unit) * unit  # equal batches: no more memory than needed
        return batch, -(-longest // batch)

    def _routed_pass(self, reads, read_len, query, hit_bits=None, counts=None):
        """One insert / query pass over this rank's reads on the routed path.  The unit of work is a JOB =
        (batch of reads, position window): route (pass A with the global geometry, the probes inside the
        window) into a send block set; the owners' bins then travel and are applied a GROUP at a time (1/8
        of a shard's level-0 bins: the unit the owner splits and applies anyway), so the receive side needs
        two groups of buffer instead of two block sets and the exchange of group g+1 overlaps the apply of
        group g.  Filters of up to 2^42 positions have one window; a 2^43-bit filter on 8 GPUs has two, each
        owned by 4 consecutive shards, and every batch is routed once per window (only the window's owners
        receive blocks of that job).  With RCCL the next job is routed on a second stream while the groups
        of this one are exchanged and applied.  Entries that could not be staged at their origin (skewed
        input) come back as explicit positions per job; they are collected without limit and exchanged once
        at the end of the pass, like the fail lists of a query."""
        shape = self._route_shape(read_len)
        batch, n_batches = self._route_batches(reads, read_len, shape)
        if n_batches == 0:
            return True
        p = _RoutedPass(self, shape, reads, read_len, query, hit_bits, batch)
        pending = None
        for j in range(n_batches * shape.n_win):
            p.route(j)
            if shape.pipelined:
                if pending is not None:
                    p.finish(pending)
                pending = j
            else:
                p.finish(j)
        if pending is not None:
            p.finish(pending)
        return p.epilogue(counts)

    # ---- gather mode ------------------------------------------------------------------------------
    GATHER_BYTES = 48 << 30  # peers' reads held per round, all peers together

    def _gather_pass(self, reads, read_len, query, hit_bits=None, counts=None):
        """One insert / query pass in gather mode.  Per round every rank contributes `chunk` bytes of its
        reads (the last one padded with 'N': no k-mers) to all peers and, while they travel, hashes its
        OWN chunk; then the peers' chunks, while the next round's are in flight.  Query: every shard
        answers "all of my probes of this window are set" for every chunk it sees, the partial bitmaps of
        the peers' chunks go back to their owners (1 bit per window and peer) and are ANDed there."""
        ops, net, W, dev, rank = self.ops, self.net, self.world, self.ops.device, self.rank
        longest = net.max(reads.numel())
        if query and counts is not None:
            counts[0] = counts[1] = 0
        if longest == 0:
            return
        # one-rank test modes: the rank is its own (only) peer, so that the collectives carry data
        peers = list(range(W)) if net.force_exchange else [p for p in range(W) if p != rank]
        own_first = not net.force_exchange
        unit = 64 * read_len
        cap = self.batch_bytes_cap or max(self.GATHER_BYTES // max(len(peers), 1), unit)
        rounds = -(-longest // cap)
        chunk = -(-(-(-longest // rounds)) // unit) * unit
        rounds = -(-longest // chunk)
        n_slots = 2 if rounds > 1 else 1
        words = chunk // 64
        gathered = [torch.empty(len(peers) * chunk, dtype=torch.uint8, device=dev) for _ in range(n_slots)] \
            if peers else []
        pad = None  # send buffer for a chunk shorter than `chunk` (a rank's last one)
        if query:
            own_part = torch.empty(words, dtype=torch.int64, device=dev)
            own_valid = torch.empty(words, dtype=torch.int64, device=dev)
            if peers:
                part = torch.empty(len(peers) * words, dtype=torch.int64, device=dev)
                # the peers count their own clean windows; only the one-rank test modes need this rank's here
                valid = None if own_first else torch.empty(len(peers) * words, dtype=torch.int64, device=dev)
                sendb = torch.zeros(W * words, dtype=torch.int64, device=dev)
                back = torch.empty(W * words, dtype=torch.int64, device=dev)
        n_valid = 0

        def start(r):
            nonlocal pad
            if not peers:
                return []
            mine = reads[r * chunk: (r + 1) * chunk]
            if mine.numel() < chunk:
                if pad is None:
                    pad = torch.empty(chunk, dtype=torch.uint8, device=dev)
                pad[: mine.numel()].copy_(mine)
                pad[mine.numel():].fill_(78)  # 'N'
                mine = pad
            return net.gather(gathered[r % n_slots], mine, peers)

        works = start(0)
        for r in range(rounds):
            mine = reads[r * chunk: (r + 1) * chunk]
            have = mine.numel()
            hw = (have + 63) // 64
            if own_first and have:  # hashed while the peers' chunks of this round arrive
                if not query:
                    ops.insert_seqs(mine, read_len)
                else:
                    ops.contains_seqs(mine, read_len, own_part, own_valid)
            for w in works:
                w.wait()
            # the next round's send buffer may be `pad`: this round's sends have completed (waited above)
            nxt = start(r + 1) if r + 1 < rounds else []
            if peers:
                buf = gathered[r % n_slots]
                if not query:
                    ops.insert_seqs(buf, read_len)
                else:
                    ops.contains_seqs(buf, read_len, part, valid)
                    # row p of sendb = my answer for rank p's chunk; row p of back = rank p's answer for mine
                    sendb.view(W, words)[peers] = part.view(len(peers), words)
                    for w in net.rows_all_to_all(back.view(W, words), sendb.view(W, words),
                                                 async_op=not net.stage_cpu):
                        w.wait()
            if query and hw:
                if own_first:
                    acc, val = own_part[:hw].clone(), own_valid
                else:
                    acc, val = None, valid.view(len(peers), words)[peers.index(rank)]
                for p in peers:
                    row = back.view(W, words)[p, :hw]
                    acc = row.clone() if acc is None else acc.bitwise_and_(row)
                hit_bits[r * words: r * words + hw].copy_(acc)
                if counts is not None:
                    n_valid += ops.popcount_bits(val[:hw])
            works = nxt
        if query:
            self._fill_counts(counts, n_valid, reads, hit_bits)

    # ---- public -----------------------------------------------------------------------------
    def insert_reads(self, reads, read_len):
        """insertSeq over this rank's uniform-length reads (flat uint8 tensor)"""
        if self.mode == "gather":
            return self._gather_pass(reads, read_len, 0)
        if self._routed():
            self._routed_pass(reads, read_len, 0)
            return
        if self.counting:
            raise RuntimeError("counting filters have no direct exchange path")
        for _, chunk in self._batches(reads, read_len):
            send, _, cnt, recv_cnt, _ = self._bucketed(chunk, read_len, False)
            mine = self.net.all_to_all(send, cnt, recv_cnt)
            self.ops.insert_positions(mine)

    def contains_reads(self, reads, read_len, hit_bits, counts=None):
        """contains() of every window of this rank's reads -> hit_bits (int64 bitmap over the whole
        buffer, bit p = window at byte p); counts (optional int64[2]) = {clean windows, hits}"""
        if self.mode == "gather":
            self._gather_pass(reads, read_len, 1, hit_bits, counts)
            return hit_bits
        if self._routed():
            if self._routed_pass(reads, read_len, 1, hit_bits, counts):
                return hit_bits
            # too many failed probes for the fail lists: fall through to the exact answer routing
            if self.counting:
                raise RuntimeError("counting query: more failed probes than the fail lists hold")
        n_valid = 0
        for off, chunk in self._batches(reads, read_len):
            send, stags, cnt, recv_cnt, valid = self._bucketed(chunk, read_len, True)
            theirs = self.net.all_to_all(send, cnt, recv_cnt)
            answers = self.ops.test_positions(theirs)
            back = self.net.all_to_all(answers, recv_cnt, cnt)  # same order as `send`
            words = valid.numel()
            w0 = off // 64  # batches are multiples of 64 bytes as long as batch_reads*read_len % 64 == 0
            if off % 64:
                raise ValueError("batch_reads * read_len must be a multiple of 64")
            view = hit_bits[w0: w0 + words]
            view.copy_(valid)
            self.ops.and_answers(stags, back, view)
            if counts is not None:
                n_valid += self.ops.popcount_bits(valid)
        self._fill_counts(counts, n_valid, reads, hit_bits)
        return hit_bits

    def store(self, path):
        """every rank writes its bit range into the one BTLBloomFilter_v1 file"""
        self.ops.store_shard(path)
        if dist.is_initialized():
            dist.barrier(self.net.group)
