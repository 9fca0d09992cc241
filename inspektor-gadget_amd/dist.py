"""Multi-GPU merges of the aggregation path.

One process per GPU.  Two transports carry the exchanges:

  * torch.distributed (default): on an "nccl" group its collectives are RCCL over xGMI on
    MI355X; on "gloo" (the CPU tests, and the ranks that share one GPU in the world-size-2
    GPU test) device tensors are staged through the host.
  * RCCL through libigx.so's igx_dist_* C ABI (the same entry points a cgo caller binds),
    with IGX_DIST=igx on an "nccl" group; torch.distributed only hands rank 0's ncclUniqueId
    to the other ranks.

Only data movement and bookkeeping live here; every aggregation and merge runs in libigx.so:

  log2 histograms (C3)      dense u32[keys][27] per rank -> all-reduce(sum)            exact
  group-by / distinct (C4)  local partial groups -> all-to-all by hash(key) -> the owner
                            merges them (igx_groupby_update_ex: SUM of partials, MIN of
                            first index) -> each key lives on exactly one rank         exact
  top-K (C2, C5)            per-rank K candidates -> all-gather -> one more top-K with
                            the global first index as the position                     exact
                            (keys are rank-disjoint after the exchange or by ingest)
  top-K by a DESC sum (C5)  topk_threshold: local top-K, groups above a threshold, then the
                            union's keys looked up on every rank -- three all-gathers of a few
                            dozen rows instead of the group exchange                   exact

The reference merges nodes by concatenating per-node arrays (snapshotcombiner.go:79-106);
an exact global merge is stricter and equal to the single-device result on the union.
"""
from __future__ import annotations

import ctypes as C
import os

from .runtime import torch_mod, context, ptr

_comm = None


def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


def world():
    """(rank, world_size); (0, 1) without an initialised process group."""
    d = _dist()
    return (d.get_rank(), d.get_world_size()) if d else (0, 1)


class TorchComm:
    """torch.distributed transport (gloo, or any backend torch supports for these calls).
    Device tensors go through the host when the backend is gloo."""

    name = "torch"

    def __init__(self, d):
        self.d = d
        self.stage = d.get_backend() == "gloo"

    def _out(self, t):
        return t.cpu() if self.stage and t.is_cuda else t

    def allreduce_u32(self, hist):
        torch = torch_mod()
        h = self._out(hist)
        self.d.all_reduce(h.view(torch.int32), op=self.d.ReduceOp.SUM)   # same bits mod 2^32
        if h is not hist:
            hist.copy_(h)
        return hist

    def allgather_rows(self, rows):
        torch = torch_mod()
        d, ws = self.d, self.d.get_world_size()
        r = self._out(rows)
        n = torch.tensor([r.shape[0]], dtype=torch.int64, device=r.device)
        ns = [torch.empty_like(n) for _ in range(ws)]
        d.all_gather(ns, n)
        counts = [int(x.item()) for x in ns]
        m = max(counts)
        pad = torch.zeros((max(1, m), r.shape[1]), dtype=r.dtype, device=r.device)
        if r.shape[0]:
            pad[: r.shape[0]] = r
        outs = [torch.empty_like(pad) for _ in range(ws)]
        d.all_gather(outs, pad)
        return torch.cat([o[:c] for o, c in zip(outs, counts)]).to(rows.device)

    def alltoallv_rows(self, rows, counts):
        torch = torch_mod()
        d = self.d
        r = self._out(rows)
        send_counts = torch.tensor(counts, dtype=torch.int64, device=r.device)
        recv_counts = torch.empty_like(send_counts)
        d.all_to_all_single(recv_counts, send_counts)
        rc = recv_counts.tolist()
        out = torch.empty((sum(rc), r.shape[1]), dtype=r.dtype, device=r.device)
        d.all_to_all_single(out, r.contiguous(), rc, list(counts))
        return out.to(rows.device)


class IgxComm:
    """RCCL transport through libigx.so (igx_dist_*).  Rank 0's ncclUniqueId reaches the
    other ranks over the torch process group; everything after that is the C ABI."""

    name = "igx"

    def __init__(self, d, timeout_ms=None):
        torch = torch_mod()
        from . import _abi
        rank, ws = d.get_rank(), d.get_world_size()
        self.h, self.ws = None, ws
        uid = (C.c_uint8 * _abi.DIST_ID_BYTES)()
        ok, err = 1, None
        try:
            self.ctx = context()
            if rank == 0:
                ok = int(self.ctx.L.igx_dist_get_unique_id(uid) == 0)
            dev = torch.device("cuda", self.ctx.device)
        except Exception as e:   # noqa: BLE001 -- still join the broadcast below, flagged
            ok, err, dev = 0, e, torch.device("cuda", torch.cuda.current_device())
        # every rank joins the broadcast whatever happened above (the last byte carries rank
        # 0's status), so no rank is left waiting in it while the others move on
        t = torch.tensor(list(uid) + [ok], dtype=torch.uint8, device=dev)
        d.broadcast(t, 0)
        v = t.cpu().tolist()
        # every rank's status, before any rank enters igx_dist_init: a rank that cannot open the
        # transport would otherwise leave its peers inside ncclCommInitRank until the deadline
        # (IGX_DIST_TIMEOUT_MS) -- now all of them raise here and select_transport falls back
        st = torch.tensor([0 if err is not None else 1], dtype=torch.int32, device=dev)
        d.all_reduce(st, op=d.ReduceOp.MIN)
        if err is not None:
            raise RuntimeError(f"IgxComm on rank {rank}: {err}")
        if not v[-1]:
            raise RuntimeError("igx_dist_get_unique_id failed on rank 0")
        if int(st.item()) == 0:
            raise RuntimeError(f"IgxComm on rank {rank}: a peer could not open the transport")
        uid = (C.c_uint8 * _abi.DIST_ID_BYTES)(*v[:-1])
        h = C.c_void_p()
        self.ctx.check(self.ctx.L.igx_dist_init(self.ctx.h, uid, ws, rank, C.byref(h)))
        self.h = h
        if timeout_ms is not None:
            self.ctx.check(self.ctx.L.igx_dist_set_timeout(self.h, int(timeout_ms)))

    def wait(self):
        """igx_dist_wait: the stream drained, bounded by the communicator's deadline (EIO and
        an aborted communicator when a peer stops answering)."""
        self.ctx.check(self.ctx.L.igx_dist_wait(self.h))

    def _bind(self):
        self.ctx.bind_stream()
        return self.ctx.L

    def allreduce_u32(self, hist):
        L = self._bind()
        self.ctx.check(L.igx_dist_allreduce_u32(self.h, ptr(hist), hist.numel()))
        self.wait()
        return hist

    def allgather_rows(self, rows):
        torch = torch_mod()
        L = self._bind()
        rows = rows.contiguous()
        n, rb = rows.shape
        counts = (C.c_uint64 * self.ws)()
        self.ctx.check(L.igx_dist_allgather_rows(self.h, ptr(rows), n, rb, None, 0, counts))   # size query
        tot = sum(counts)
        out = torch.empty((max(1, tot), rb), dtype=rows.dtype, device=rows.device)
        self.ctx.check(L.igx_dist_allgather_rows(self.h, ptr(rows), n, rb, ptr(out), tot, counts))
        self.wait()
        return out[:tot]

    def alltoallv_rows(self, rows, counts):
        torch = torch_mod()
        L = self._bind()
        rows = rows.contiguous()
        rb = rows.shape[1]
        sc = (C.c_uint64 * self.ws)(*counts)
        rc = (C.c_uint64 * self.ws)()
        self.ctx.check(L.igx_dist_alltoallv_rows(self.h, ptr(rows), sc, rb, None, 0, rc))   # size query
        tot = sum(rc)
        out = torch.empty((max(1, tot), rb), dtype=rows.dtype, device=rows.device)
        self.ctx.check(L.igx_dist_alltoallv_rows(self.h, ptr(rows), sc, rb, ptr(out), tot, rc))
        self.wait()
        return out[:tot]

    def barrier(self):
        self.ctx.check(self._bind().igx_dist_barrier(self.h))

    def close(self):
        if self.h:
            self.ctx.L.igx_dist_destroy(self.h)
            self.h = None


def comm():
    """The transport for the current process group (None without one): the one
    select_transport() agreed on, else torch's own collectives (on an "nccl" group these are
    RCCL over xGMI too), or the igx_dist_* C ABI when IGX_DIST=igx on an nccl group.
    bench.py selects the C ABI at N > 1 (select_transport("igx")); the library's default stays
    torch's collectives until a world >= 2 run on GPUs has checked the C ABI's send/recv loops
    (their planning, igx_dist_plan_*, is tested for 2..8 ranks against gloo)."""
    global _comm
    d = _dist()
    if d is None or d.get_world_size() == 1:
        return None
    if _comm is None:
        use_igx = d.get_backend() == "nccl" and os.environ.get("IGX_DIST", "torch") == "igx"
        _comm = IgxComm(d) if use_igx else TorchComm(d)
    return _comm


def select_transport(prefer="igx"):
    """Pick the transport every rank will use, agreed over the process group: prefer="igx"
    tries the igx_dist_* C ABI (RCCL) on an "nccl" group; if any rank's igx_dist_init fails,
    every rank falls back to torch's collectives.  Returns the transport's name ("igx" or
    "torch"), or None without a multi-rank group."""
    global _comm
    d = _dist()
    if d is None or d.get_world_size() == 1:
        return None
    shutdown()
    c, ok = None, 1
    if prefer == "igx" and d.get_backend() == "nccl":
        try:
            c = IgxComm(d)
        except Exception:   # noqa: BLE001 -- any local failure: agree on the fallback below
            c, ok = None, 0
        torch = torch_mod()
        flag = torch.tensor([ok], dtype=torch.int32,
                            device=torch.device("cuda", torch.cuda.current_device()))
        d.all_reduce(flag, op=d.ReduceOp.MIN)
        if int(flag.item()) == 0 and c is not None:
            c.close()
            c = None
    _comm = c if c is not None else TorchComm(d)
    return _comm.name


def shutdown():
    """Release the RCCL communicator (before destroy_process_group)."""
    global _comm
    if _comm is not None and hasattr(_comm, "close"):
        _comm.close()
    _comm = None


def allreduce_hist(hist, c=None):
    """C3: in-place sum of a u32 histogram over ranks (c: a transport; default comm())."""
    c = c or comm()
    return hist if c is None else c.allreduce_u32(hist)


def allgather_rows(rows, c=None):
    """Concatenate every rank's (n_r, row_bytes) uint8 rows in rank order (n_r may differ)."""
    c = c or comm()
    return rows if c is None else c.allgather_rows(rows)


def partition_by_owner(rows, key_bytes, ws):
    """Group packed rows by the rank that owns their key (igx_partition_rows on the device:
    FNV-1a over the key's u32 words mod ws, stable).  Returns (rows, counts per rank)."""
    from . import engine
    return engine.partition_rows(rows, key_bytes, ws)


def exchange_partitioned(rows, counts, c=None):
    """All-to-all of rows already grouped by destination rank (counts[r] rows for rank r,
    in rank order; rows past their sum are ignored).  Returns the rows this rank owns, in
    source-rank order.  Negative counts are igx_partition_groups' overflow sentinel (the table
    listed more groups than the partition's output holds, so the rows are truncated): IgxError
    with IGX_ENOSPC, before anything is sent."""
    if any(int(n) < 0 for n in counts):
        from . import _abi
        raise _abi.IgxError(_abi.IGX_ENOSPC, "exchange_partitioned: the partitioned table held more groups than "
                                             "its capacity (igx_partition_groups' counts are -1): rows truncated")
    c = c or comm()
    rows = rows[:sum(counts)]
    return rows if c is None else c.alltoallv_rows(rows, counts)


def owner_capacity(capacity, ws, slack=1.25):
    """Groups an owner table must hold when `capacity` bounds the distinct keys of the whole
    (global) interval: keys reach their owner by a hash of the key, so an owner holds about
    1/ws of them; slack covers the hash's imbalance (at 1M keys per owner its spread is
    ~0.1 %)."""
    return min(capacity, int(capacity * slack / ws) + 4096)


def exchange_rows(rows, key_bytes):
    """C4 group-by exchange: every partial-group row goes to the rank owning its key."""
    r, ws = world()
    if ws == 1:
        return rows
    part, counts = partition_by_owner(rows, key_bytes, ws)
    return exchange_partitioned(part, counts)


def unpack_rows(rows, key_widths, naggs):
    """Packed group rows (key padded to 4-byte columns | naggs x u64 | first u64) -> SoA
    tensors: key columns (u8 (n, w) for byte keys, typed for 1/2/4/8), aggregates, first."""
    from . import engine
    torch = torch_mod()
    typed = {1: torch.uint8, 2: torch.uint16, 4: torch.uint32, 8: torch.uint64}
    fields, o = [], 0
    for i, w in enumerate(key_widths):
        fields.append((i, o, w, typed.get(w)))
        o += (w + 3) // 4 * 4
    nk = len(key_widths)
    fields += [(nk + x, o + 8 * x, 8, torch.uint64) for x in range(naggs + 1)]
    # the rows cut into columns in one pass on the device (igx_ingest_aos, the wire-format
    # ingest's kernel), not one strided torch copy per field, each re-reading every row
    r8 = rows.contiguous().view(torch.uint8)   # (n, row bytes)
    cols = {}
    for f0 in range(0, len(fields), 16):   # igx_ingest_aos takes up to 16 fields a call
        cols.update(engine.ingest_aos(r8, r8.shape[0], r8.shape[1], fields[f0:f0 + 16]))
    outs = [cols[i] for i in range(len(fields))]
    return outs[:nk], outs[nk:nk + naggs], outs[nk + naggs]


def owner_table(key_widths, out_widths, capacity):
    """The owner's merge table: SUM of the partials per aggregate, first = MIN, in the cached
    form (a wide table, capacity past the 4 GiB of key records a cached table addresses: AUTO's
    partitioned form).  A merge's rows are nearly all LDS misses (each key arrives once per rank that saw it),
    which would send AUTO to the partitioned form; but the cached form keeps the owner's keys
    across intervals and finds them, and measures faster (profiles/r06/emulated_rank8_*.json,
    rank 0 of 8: C4 0.98 -> 0.62 ms, C5 1.67 -> 1.53 ms)."""
    from . import _abi, engine
    nk = len(key_widths)
    spec = [_abi.Agg(_abi.AGG_SUM, nk + x, _abi.NO_COL, ow, 0) for x, ow in enumerate(out_widths)]
    t = engine.Table(key_widths, spec, max(1, capacity))
    _prefer_cached(t)
    return t


def _prefer_cached(table):
    """The cached form where the table has one.  A wide table (key records of 4 GiB or more, see
    igx_groupby_create) does not: it stays in AUTO, which runs every interval partitioned."""
    from . import _abi
    try:
        table.set_mode(_abi.GB_CACHED)
    except _abi.IgxError as e:
        if e.code != _abi.IGX_ENOTSUP:
            raise


def merge_partials(rows, key_widths, out_widths, capacity, table=None, sync=True):
    """Owner-side merge of exchanged partial groups on the device: one igx table whose
    aggregates SUM the partials and whose first index is the MIN of the partials' (the
    rows' u64 first column drives igx_groupby_update_ex's index column).  Returns the
    engine.Table, finalized (`table`, when given, is reset and reused; sync=False leaves the
    group count on the device, igx_groupby_finalize_async)."""
    from . import _abi, engine
    kcols, aggs, first = unpack_rows(rows, key_widths, len(out_widths))
    nk = len(kcols)
    if table is None:
        spec = [_abi.Agg(_abi.AGG_SUM, nk + x, _abi.NO_COL, ow, 0) for x, ow in enumerate(out_widths)]
        table = engine.Table(key_widths, spec, max(1, capacity))
        _prefer_cached(table)   # see owner_table()
    else:
        table.reset()
    n = rows.shape[0]
    if n:
        table.update(kcols + aggs + [first], list(range(nk)), n, 0, idx_col=nk + len(aggs))
    table.finalize(sync=sync)
    return table


def merge_topk(cand, key_bytes, naggs, sort_keys, k, c=None):
    """Exact global top-K from all ranks' candidate rows (key | aggs | first): all-gather,
    then igx_topk with the global first index as the position.  sort_keys:
    [(agg_index, desc)] in sortBy order."""
    from . import engine
    torch = torch_mod()
    allc = allgather_rows(cand, c)
    if allc.shape[0] == 0:
        return allc
    o = key_bytes
    keys = [(allc[:, o + 8 * x:o + 8 * x + 8].contiguous().view(torch.uint64).flatten(), desc)
            for x, desc in sort_keys]
    first = allc[:, o + 8 * naggs:o + 8 * naggs + 8].contiguous().view(torch.uint64).flatten()
    idx = engine.sort_perm(keys, allc.shape[0], pos=first, k=k)
    return engine.take([allc], idx)[0]


# ------------------------------------------------------------------------------------
# exact top-K across ranks by threshold instead of a full group exchange
# ------------------------------------------------------------------------------------
# "Top K by a DESC sum of non-negative partials" does not need every partial group at its owner:
# three small rounds (TPUT-style) give the same K rows, ties at the K-th value included.
#   round 1  local top-K rows, all-gathered, merged by key: tau = the K-th largest merged value
#            (a lower bound of the global K-th value: partial sums only grow)
#   round 2  every rank lists its groups with a local value >= T = ceil(tau / ws)
#            (igx_groupby_select_ge); their keys' union U holds every group whose global value
#            is >= tau: a group outside U has every local value < tau / ws, so its sum is < tau
#   round 3  every rank reports what it holds for U's keys (igx_groupby_lookup); merged by key
#            (SUM, MIN of first) these are U's exact global rows; their top-K is the answer
# The rounds are transport-free functions over packed rows; topk_threshold joins them with
# allgather_rows, topk_threshold_ranks plays N ranks in one process by concatenation.
U64_MAX = (1 << 64) - 1


def _key_bytes(key_widths):
    return sum((w + 3) // 4 * 4 for w in key_widths)


def _agg_host(rows, kb, x):
    """aggregate x of packed rows as a host u64 array"""
    import numpy as np
    a = rows[:, kb + 8 * x:kb + 8 * x + 8].contiguous().cpu().numpy()
    return a.copy().view(np.uint64).ravel()


def group_rows(table):
    """Every group of a finalized table as packed rows (key | aggregates | first index)."""
    torch = torch_mod()
    fin = table.fin
    G = fin["n_groups"]
    if G is None:
        G = table.wait()
    slots = torch.empty(max(1, G), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))[:G]
    if G:
        table.ctx.check(table.ctx.L.igx_memcpy_d2d(table.ctx.h, ptr(slots), C.c_void_p(fin["groups_ptr"]), G * 4))
    return table.gather(slots)


def tt_applies(table, sort_keys):
    """None when the threshold protocol can answer this sort spec on this table, else why not:
    the first sort key must be a DESC aggregate (COUNT or SUM: non-negative partials whose sum
    is the global value) that does not wrap below 8 bytes."""
    from . import _abi
    if not sort_keys:
        return "no sort key"
    src, what, desc = sort_keys[0]
    if src != _abi.TSRC_AGG:
        return "the first sort key is not an aggregate"
    if not desc:
        return "the first sort key is ascending"
    if table.out_widths[int(what or 0)] != 8:
        return "the first sort key's aggregate wraps below 8 bytes"
    return None


def tt_candidates(table, sort_keys, k):
    """Round 1, per rank: the local top-K as packed rows (the table is synchronously finalized)."""
    if table.fin["n_groups"] is None:
        table.wait()
    return table.gather(table.sort(sort_keys, k))


def tt_threshold(cand, ws, sort_keys, k, key_widths, out_widths, table=None):
    """Round 1, every rank alike: all ranks' candidates -> the decision.  {"path": "threshold",
    "tau", "T"} or {"path": "full", "reason"}: a global sum that could wrap (the largest local
    value M > (2^64 - 1) // ws), fewer than k candidate groups (then there are fewer than k
    groups in all), or tau == 0 (T would select every group).  table: a merge table to reuse."""
    import numpy as np
    torch = torch_mod()
    x, kb = int(sort_keys[0][1] or 0), _key_bytes(key_widths)
    if cand.shape[0] < 1:
        return {"path": "full", "reason": "fewer than k groups", "tau": None}
    merged = merge_partials(cand, key_widths, out_widths, max(1, cand.shape[0]), table=table)
    try:
        # the candidates' local values and the merged values in one host read
        both = torch.cat([cand, group_rows(merged)])
    finally:
        if table is None:
            merged.destroy()
    v = _agg_host(both, kb, x)
    M, vals = int(v[:cand.shape[0]].max()), np.sort(v[cand.shape[0]:])[::-1]
    if M > U64_MAX // ws:
        return {"path": "full", "reason": "a global sum could wrap 2^64", "tau": None}
    if len(vals) < k:
        return {"path": "full", "reason": "fewer than k groups", "tau": None}
    tau = int(vals[k - 1])
    if tau == 0:
        return {"path": "full", "reason": "tau == 0", "tau": 0}
    return {"path": "threshold", "tau": tau, "T": -(-tau // ws)}


def tt_select(table, sort_keys, T, cand_cap):
    """Round 2, per rank: (slots, count) of the groups whose first-sort-key value is >= T;
    count > cand_cap means the list is cut and every rank must fall back."""
    return table.select_ge(int(sort_keys[0][1] or 0), T, cand_cap)


def tt_count_row(count, device):
    """A rank's round-2 count as the one 8-byte row it all-gathers first."""
    torch = torch_mod()
    return torch.tensor([count], dtype=torch.int64, device=device).view(torch.uint8).reshape(1, 8)


def tt_counts(count_rows):
    """The all-gathered count rows -> [count per rank]."""
    torch = torch_mod()
    return [int(v) for v in count_rows.contiguous().cpu().view(torch.int64).ravel().tolist()]


def tt_union(sel, key_widths, out_widths, table=None):
    """Round 2, every rank alike: all ranks' selected rows -> one row per distinct key (the
    union U; only the keys are used)."""
    merged = merge_partials(sel, key_widths, out_widths, max(1, sel.shape[0]), table=table)
    try:
        return group_rows(merged).clone()
    finally:
        if table is None:
            merged.destroy()


def tt_lookup(table, union):
    """Round 3, per rank: this rank's rows for U's keys (the keys it does not hold dropped)."""
    rows, found = table.lookup(union)
    return rows[found.bool()]


def tt_final(rows, sort_keys, k, key_widths, out_widths, table=None):
    """Round 3, every rank alike: all ranks' rows for U (or, on the full path, the owners'
    candidates) merged by key -- SUM of the partials, MIN of the first indices -- and their
    top-K under the whole sort spec, as packed rows."""
    merged = merge_partials(rows, key_widths, out_widths, max(1, rows.shape[0]), table=table)
    try:
        return merged.gather(merged.sort(sort_keys, k)).clone()
    finally:
        if table is None:
            merged.destroy()


def topk_scratch(key_widths, out_widths, ws, k, cand_cap):
    """The three small merge tables of the protocol, to reuse across steps (without them every
    call creates and frees its own): {"r1", "r2", "r3"} for tt_threshold, tt_union, tt_final."""
    return {"r1": owner_table(key_widths, out_widths, ws * k),
            "r2": owner_table(key_widths, out_widths, ws * cand_cap),
            "r3": owner_table(key_widths, out_widths, ws * cand_cap)}


def _threshold_rounds(tables, ws, join, full, sort_keys, k, key_widths, out_widths, cand_cap, scratch):
    """The protocol over the ranks this process plays (tables) and `join`, which turns their
    per-rank rows into all ranks' rows; full(reason, tau) runs the full exchange instead."""
    s = scratch or {}
    why = tt_applies(tables[0], sort_keys)
    if why:
        return full(why, None)
    dec = tt_threshold(join([tt_candidates(t, sort_keys, k) for t in tables]), ws, sort_keys, k, key_widths,
                       out_widths, table=s.get("r1"))
    if dec["path"] == "full":
        return full(dec["reason"], dec["tau"])
    sel = [tt_select(t, sort_keys, dec["T"], cand_cap) for t in tables]
    dev = sel[0][0].device
    counts = tt_counts(join([tt_count_row(n, dev) for _, n in sel]))
    if max(counts) > cand_cap:   # the same counts on every rank: the same decision
        return full(f"a rank selected more than cand_cap={cand_cap} groups", dec["tau"])
    union = tt_union(join([t.gather(sl) for t, (sl, _) in zip(tables, sel)]), key_widths, out_widths,
                     table=s.get("r2"))
    rows = tt_final(join([tt_lookup(t, union) for t in tables]), sort_keys, k, key_widths, out_widths,
                    table=s.get("r3"))
    return rows, {"path": "threshold", "reason": None, "tau": dec["tau"], "T": dec["T"], "sent": counts,
                  "union": int(union.shape[0]), "cand_cap": cand_cap}


def topk_threshold(table, sort_keys, k, key_widths, out_widths, capacity, cand_cap=None, c=None, scratch=None):
    """Exact global top-K of a per-rank partial table (synchronously finalized) under sort_keys
    ([(src, what, desc)] as Table.sort takes them), on every rank the same packed rows (key |
    aggregates | global first index): what exchange_rows -> merge_partials -> the owner's top-K
    -> merge_topk gives, from three all-gathers of a few dozen rows (see above) when the first
    sort key is a DESC COUNT / SUM aggregate of out_width 8; any other sort spec, a possible
    wrap, fewer than k groups, tau == 0 or a rank selecting more than cand_cap (default
    max(4096, 64 k)) groups takes the full exchange (capacity: the owner table's).  Returns
    (rows, info): info["path"] is "threshold", "full" (with "reason") or, without a multi-rank
    group, "local"; "tau", "sent" (rows per rank in round 2) and "union" (|U|) describe the
    threshold path.  scratch: topk_scratch() tables to reuse."""
    c = c or comm()
    if cand_cap is None:
        cand_cap = max(4096, 64 * k)
    if c is None:
        return tt_candidates(table, sort_keys, k), {"path": "local", "reason": None, "tau": None, "sent": None,
                                                    "union": None}
    ws = world()[1]
    kb = _key_bytes(key_widths)

    def full(reason, tau):
        part, counts = partition_by_owner(group_rows(table), kb, ws)
        mine = exchange_partitioned(part, counts, c)
        own = merge_partials(mine, key_widths, out_widths, capacity)
        try:
            cand = own.gather(own.sort(sort_keys, k))
            # the owners' candidates are key-disjoint: merging them by key changes no row, and
            # its top-K is merge_topk's under sort specs with key columns too
            rows = tt_final(allgather_rows(cand, c), sort_keys, k, key_widths, out_widths)
        finally:
            own.destroy()
        return rows, {"path": "full", "reason": reason, "tau": tau, "sent": None, "union": None}

    return _threshold_rounds([table], ws, lambda parts: allgather_rows(parts[0], c), full, sort_keys, k,
                             key_widths, out_widths, cand_cap, scratch)


def topk_threshold_ranks(tables, sort_keys, k, key_widths, out_widths, capacity, cand_cap=None, scratch=None):
    """topk_threshold with one process playing every rank: tables are the ranks' partial
    tables (synchronously finalized), and the all-gathers are concatenations in rank order (the
    full exchange: every rank's groups merged in one table of `capacity`).  Same (rows, info)."""
    torch = torch_mod()
    ws = len(tables)
    if cand_cap is None:
        cand_cap = max(4096, 64 * k)
    if ws == 1:
        return tt_candidates(tables[0], sort_keys, k), {"path": "local", "reason": None, "tau": None,
                                                        "sent": None, "union": None}

    def full(reason, tau):
        own = merge_partials(torch.cat([group_rows(t) for t in tables]), key_widths, out_widths, capacity)
        try:
            rows = own.gather(own.sort(sort_keys, k)).clone()
        finally:
            own.destroy()
        return rows, {"path": "full", "reason": reason, "tau": tau, "sent": None, "union": None}

    return _threshold_rounds(tables, ws, torch.cat, full, sort_keys, k, key_widths, out_widths, cand_cap, scratch)
