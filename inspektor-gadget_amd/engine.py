"""Thin tensor-level wrappers over the igx C ABI (device tensors in, device tensors out).

The reference-shaped API (columns / filter / sort / group / top / gadgets) is built on
these.  Everything here enqueues libigx.so kernels on torch's current stream.
"""
import ctypes as C
import os
import math

from . import _abi
from ._abi import Agg, Col, Pred, SortKey, TableView, IgxError
from .runtime import context, ptr, col_of, dtype_kind, torch_mod

# ------------------------------------------------------------------------------------
# synthetic streams; bit-identical with the CPU oracle
# ------------------------------------------------------------------------------------
TCP_FIELDS = (("saddr", "u8x16"), ("daddr", "u8x16"), ("mntns", "u64"), ("pid", "u32"),
              ("comm", "u8x16"), ("lport", "u16"), ("dport", "u16"), ("family", "u16"),
              ("size", "u32"), ("dir", "u8"))
OPEN_FIELDS = (("pid", "u32"), ("uid", "u32"), ("mntns", "u64"), ("comm", "u8x16"),
               ("ret", "i64"), ("fd", "i64"), ("err", "i64"), ("path", "u32"))
BIO_FIELDS = (("dev", "u32"), ("cont", "u32"), ("delta", "i64"))
NP_FIELDS = (("src", "u32"), ("peer", "u32"), ("port", "u16"), ("pkt", "u8"), ("type", "u8"),
             ("proto", "u8"), ("hostip", "u32"), ("raddr", "u32"))
FILE_FIELDS = (("inode", "u64"), ("dev", "u32"), ("pid", "u32"), ("tid", "u32"), ("op", "u8"),
               ("count", "u32"))


def zipf_cdf(G: int, s: float):
    """Host table for the generators: u63 fixed-point CDF thresholds of Zipf(s) over ranks
    1..G (last == 1 << 63); k_gen.hip draws a rank by binary search of a u63 uniform."""
    import numpy as np
    k = np.arange(1, G + 1, dtype=np.float64)
    c = np.cumsum(k ** (-s))
    c /= c[-1]
    out = np.minimum(np.floor(c * float(1 << 63)), float(1 << 63)).astype(np.uint64)
    out[-1] = np.uint64(1 << 63)
    return out


def lognormal_quantiles(mu: float, sigma: float, nq: int = 4096, cap: int = 1 << 40):
    """Host table for igx_gen_bio: nq+1 monotone quantile boundaries (u64 ns) of
    lognormal(mu, sigma), capped (SURVEY.md §8(d) C3 latencies)."""
    import numpy as np
    from scipy.stats import norm
    p = (np.arange(nq + 1, dtype=np.float64) + 0.5) / (nq + 1)
    q = np.minimum(np.exp(mu + sigma * norm.ppf(p)), float(cap))
    return np.maximum.accumulate(np.floor(q)).astype(np.uint64)


def _alloc(fields, n, device):
    torch = torch_mod()
    dt = {"u8": torch.uint8, "u16": torch.uint16, "u32": torch.uint32, "u64": torch.uint64,
          "i64": torch.int64}
    out = {}
    for name, f in fields:
        if f == "u8x16":
            out[name] = torch.empty((n, 16), dtype=torch.uint8, device=device)
        else:
            out[name] = torch.empty(n, dtype=dt[f], device=device)
    return out


def perm_params(G):
    A = 999983
    while math.gcd(A, G) != 1:
        A += 2
    return (A % G, 12345 % G) if G > 1 else (1, 0)


def gen_tcp(seed, rank, G, cdf, base, n, out=None):
    ctx = context()
    ev = out or _alloc(TCP_FIELDS, n, cdf.device)
    A, B = perm_params(G)
    ctx.check(ctx.L.igx_gen_tcp(ctx.h, seed, rank, G, A, B, ptr(cdf), base, n,
                                *[ptr(ev[k]) for k, _ in TCP_FIELDS]))
    return ev


def gen_open(seed, comm_cdf, base, n):
    ctx = context()
    ev = _alloc(OPEN_FIELDS, n, comm_cdf.device)
    ctx.check(ctx.L.igx_gen_open(ctx.h, seed, ptr(comm_cdf), base, n,
                                 *[ptr(ev[k]) for k, _ in OPEN_FIELDS]))
    return ev


def gen_bio(seed, q, base, n):
    ctx = context()
    ev = _alloc(BIO_FIELDS, n, q.device)
    ctx.check(ctx.L.igx_gen_bio(ctx.h, seed, ptr(q), q.numel() - 1, base, n,
                                *[ptr(ev[k]) for k, _ in BIO_FIELDS]))
    return ev


def gen_np(seed, nsrc, npeer, base, n, device="cuda"):
    ctx = context()
    ev = _alloc(NP_FIELDS, n, device)
    ctx.check(ctx.L.igx_gen_np(ctx.h, seed, nsrc, npeer, base, n,
                               *[ptr(ev[k]) for k, _ in NP_FIELDS]))
    return ev


def gen_file(seed, rank, G, cdf, base, n):
    ctx = context()
    ev = _alloc(FILE_FIELDS, n, cdf.device)
    A, B = perm_params(G)
    ctx.check(ctx.L.igx_gen_file(ctx.h, seed, rank, G, A, B, ptr(cdf), base, n,
                                 *[ptr(ev[k]) for k, _ in FILE_FIELDS]))
    return ev


# ------------------------------------------------------------------------------------
# filter
# ------------------------------------------------------------------------------------
def filter_rows(cols, preds, n, valid=None, any=False, nil_match=False, device_count=False):
    """cols: list of device tensors (indexed by Pred.col); preds: list of Pred.
    any=False: AND (MatchAll); any=True: OR (MatchAny); any number of preds.
    nil_match=False: nil rows (valid == 0) are skipped (FilterEntries, filter.go:310-314);
    True: a nil row evaluates Match(nil) == negate per pred (filter.go:286-291).
    Returns (idx u32 tensor of length n_selected); with device_count=True, (idx of capacity n,
    count u64 device tensor) and no host synchronisation."""
    torch = torch_mod()
    ctx = context()
    dev = cols[0].device if cols else (valid.device if valid is not None else "cuda")
    ccols = (Col * max(1, len(cols)))(*[col_of(t, dtype_kind(t)) for t in cols])
    cpreds = (Pred * max(1, len(preds)))(*preds)
    out = torch.empty(max(1, n), dtype=torch.uint32, device=dev)
    cnt = torch.zeros(1, dtype=torch.uint64, device=dev)
    flags = (_abi.FILTER_ANY if any else 0) | (_abi.FILTER_NIL_MATCH if nil_match else 0)
    ctx.check(ctx.L.igx_filter_ex(ctx.h, ccols, len(cols), cpreds, len(preds), ptr(valid), n, flags,
                                  ptr(out), ptr(cnt)))
    if device_count:
        return out, cnt
    k = int(cnt.item())
    return out[:k]


def take(tensors, idx, nrows=None, pad=False):
    """igx_take: rows idx (device u32/int32/int64) of every tensor ((n,) or (n, W)) gathered
    on the device into fresh tensors of the same dtypes -- the compacted batch FilterEntries
    returns (filter.go:294-325).  Ids >= nrows yield zero rows; pad=True marks the callers
    that rely on it (the padded top-K merge), and IGX_DEBUG_TAKE=1 makes every other call
    raise IndexError on such an id."""
    torch = torch_mod()
    ctx = context()
    if idx.dtype not in (torch.int32, torch.uint32):
        idx = idx.to(torch.int32)
    idx = idx.contiguous()
    k = int(idx.numel())
    tensors = [t.contiguous() for t in tensors]
    outs = [torch.empty((k,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in tensors]
    if k and tensors:
        n = int(tensors[0].shape[0]) if nrows is None else nrows
        if not pad and os.environ.get("IGX_DEBUG_TAKE"):
            # debug assert (one host sync): igx_take zero-fills ids >= nrows, which only the
            # padded top-K merge relies on; the torch index_select it replaced raised here
            hi = int(idx.to(torch.int64).max())
            if hi >= n or int(idx.to(torch.int64).min()) < 0:
                raise IndexError(f"take: row id {hi} out of range for {n} rows")
        ccols = (Col * len(tensors))(*[col_of(t, dtype_kind(t), t[0].numel() * t.element_size() if t.dim() > 1 else None)
                                         for t in tensors])
        dst = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        ctx.check(ctx.L.igx_take(ctx.h, ccols, len(tensors), n, ptr(idx), k, dst))
    return outs


# ------------------------------------------------------------------------------------
# sort
# ------------------------------------------------------------------------------------
def sort_perm(keys, n, pos=None, valid=None, k=None, rowmap=None, d_count=None):
    """keys: list of (tensor, desc) in sortBy order.  Returns u32 permutation (first k).
    rowmap (u32, n rows): sort the selection vector -- row i is row rowmap[i] of the key
    columns, valid and pos (igx_sort_perm_ex); the result is then rowmap values in order.
    d_count (u64 device tensor, with rowmap): the slice is rowmap[:d_count], n its upper bound
    (igx_sort_perm_dn: no host round trip); the result has capacity n, its first d_count
    entries sorted."""
    torch = torch_mod()
    ctx = context()
    dev = keys[0][0].device if keys else (pos.device if pos is not None else "cuda")
    sk = []
    for key in keys:
        t, desc = key[0], key[1]
        kind = key[2] if len(key) > 2 else dtype_kind(t)
        width = t.shape[1] if t.dim() == 2 else t.element_size()
        sk.append(SortKey(C.c_void_p(t.data_ptr()), width, kind, 1 if desc else 0, 0))
    arr = (SortKey * max(1, len(sk)))(*sk)
    m = n if k is None else min(k, n)
    out = torch.empty(max(1, m), dtype=torch.uint32, device=dev)
    if n == 0:
        return out[:0]
    if rowmap is not None:
        if k is not None:
            raise ValueError("a top-K over a selection vector: sort the view first")
        if d_count is not None:
            ctx.check(ctx.L.igx_sort_perm_dn(ctx.h, arr, len(sk), n, ptr(d_count), ptr(pos), ptr(valid),
                                             ptr(rowmap), ptr(out)))
        else:
            ctx.check(ctx.L.igx_sort_perm_ex(ctx.h, arr, len(sk), n, ptr(pos), ptr(valid), ptr(rowmap), ptr(out)))
    elif k is None:
        ctx.check(ctx.L.igx_sort_perm(ctx.h, arr, len(sk), n, ptr(pos), ptr(valid), ptr(out)))
    else:
        if valid is not None:
            raise ValueError("topk does not take a nil mask")
        ctx.check(ctx.L.igx_topk(ctx.h, arr, len(sk), n, ptr(pos), m, ptr(out)))
    return out[:m]


sort_perm_kinds = sort_perm


# ------------------------------------------------------------------------------------
# group-by table
# ------------------------------------------------------------------------------------
class Table:
    """igx_table: keyed aggregation with first-occurrence tracking.

    capacity (at most 2^28) bounds the interval's distinct keys.  A table whose key records
    reach 4 GiB (slots x key stride, e.g. more than 8.39M groups of top tcp's key) is *wide*:
    it runs the direct and partitioned forms only (see igx_groupby_create in include/igx.h)."""

    def __init__(self, key_widths, aggs, capacity, ctx=None):
        self.ctx = context() if ctx is None else ctx
        kw = (C.c_uint32 * len(key_widths))(*key_widths)
        ca = (Agg * max(1, len(aggs)))(*aggs)
        h = C.c_void_p()
        self.ctx.check(self.ctx.L.igx_groupby_create(self.ctx.h, kw, len(key_widths), ca,
                                                     len(aggs), capacity, C.byref(h)))
        self.h = h
        self.key_widths = list(key_widths)
        self.naggs = len(aggs)
        self.out_widths = [int(a.out_width) or 8 for a in aggs]
        self.capacity = capacity

    def update(self, cols, key_cols, n, base_idx=0, preds=(), valid=None, idx_col=None):
        """igx_groupby_update_ex: rows [0,n) of cols; valid (u8) masks rows out; idx_col is
        the index of a u64 column of global event indices (merging partial groups)."""
        ctx = self.ctx
        ctx.bind_stream()
        ccols = (Col * len(cols))(*[col_of(t, dtype_kind(t)) for t in cols])
        kc = (C.c_uint32 * len(key_cols))(*key_cols)
        cp = (Pred * max(1, len(preds)))(*preds)
        ctx.check(ctx.L.igx_groupby_update_ex(self.h, ccols, len(cols), kc, cp, len(preds),
                                              ptr(valid), _abi.NO_COL if idx_col is None else idx_col,
                                              n, base_idx))

    def wait(self):
        """igx_groupby_wait: the group count of the last finalize(sync=False), with its status
        (IGX_ENOSPC raises as finalize would have)."""
        n = C.c_uint64()
        self.ctx.check(self.ctx.L.igx_groupby_wait(self.h, C.byref(n)))
        if getattr(self, "fin", None) is not None:
            self.fin["n_groups"] = n.value
        return n.value

    def info(self):
        """igx_groupby_info: the current interval's form and AUTO's plan, as a dict."""
        from ._abi import GroupbyInfo
        v = GroupbyInfo()
        self.ctx.check(self.ctx.L.igx_groupby_info(self.h, C.byref(v)))
        return {f: getattr(v, f) for f, _ in GroupbyInfo._fields_ if f != "pad"}

    def log_stats(self):
        """igx_groupby_log_stats: the update log's counters of the last collected finalize's
        interval (logged records and the three fallback counts), as a dict."""
        from ._abi import GroupbyLogStats
        v = GroupbyLogStats()
        self.ctx.check(self.ctx.L.igx_groupby_log_stats(self.h, C.byref(v)))
        return {f: getattr(v, f) for f, _ in GroupbyLogStats._fields_}

    def rowplan(self):
        """igx_groupby_rowplan: the row plan the last cached update ran (0 general, 1 top tcp,
        2 top file)."""
        return int(self.ctx.L.igx_groupby_rowplan(self.h))

    def reset(self):
        self.ctx.check(self.ctx.L.igx_groupby_reset(self.h))

    def set_mode(self, mode):
        """igx_groupby_set_mode: _abi.GB_AUTO (default), GB_CACHED, GB_DIRECT or GB_PART.
        GB_CACHED on a wide table raises IgxError (code IGX_ENOTSUP) with the library's message;
        the table keeps its mode."""
        self.ctx.check(self.ctx.L.igx_groupby_set_mode(self.h, mode))

    def finalize(self, sync=True):
        """Returns the table view (raw device pointers, slot-indexed) as a dict; `groups_ptr`
        lists the n_groups occupied slots.  sync=True synchronises (igx_groupby_finalize);
        sync=False leaves the group count on the device (igx_groupby_finalize_async:
        n_groups is None until wait(), and a top-K sort reads the count on the device)."""
        v = TableView()
        if sync:
            self.ctx.check(self.ctx.L.igx_groupby_finalize(self.h, C.byref(v)))
        else:
            self.ctx.check(self.ctx.L.igx_groupby_finalize_async(self.h, C.byref(v)))
        self._view = v
        self.fin = {"n_groups": v.n_groups if sync else None, "n_slots": v.n_slots, "key_bytes": v.key_bytes,
                    "key_stride": v.key_stride, "val_stride": v.val_stride, "keys_ptr": v.keys,
                    "aggs_ptr": [v.aggs[i] for i in range(v.naggs)], "first_ptr": v.first_idx,
                    "groups_ptr": v.groups, "d_n_groups": v.d_n_groups}
        return self.fin

    def sort(self, keys, k=0):
        """igx_groupby_sort: keys = [(src, index_or_(offset,width,kind), desc)].  Returns the
        first k (0 = all) group slots in SortStats order (device u32)."""
        torch = torch_mod()
        ts = []
        for src, what, desc in keys:
            if src == _abi.TSRC_KEY:
                off, w, kind = what
                ts.append(_abi.TSortKey(src, 0, off, w, kind, int(desc)))
            elif src == _abi.TSRC_IPTEXT:
                addr_off, fam_off = what
                ts.append(_abi.TSortKey(src, fam_off, addr_off, 16, _abi.KIND_BYTES, int(desc)))
            else:
                ts.append(_abi.TSortKey(src, int(what or 0), 0, 0, 0, int(desc)))
        arr = (_abi.TSortKey * max(1, len(ts)))(*ts)
        G = self.fin["n_groups"]
        if G is None:   # finalize(sync=False): a top-K over integer keys reads the count on the device
            dev_ok = 0 < k <= 4096 and 2 * k < self.capacity and all(t.src != _abi.TSRC_IPTEXT and not (t.src == _abi.TSRC_KEY and
                                                                             t.kind == _abi.KIND_FLOAT) for t in ts)
            if not dev_ok:
                G = self.wait()
        # without the count, k slots come back; those past the group count are 0xFFFFFFFF
        # (gather() turns them into zero rows)
        m = k if G is None else (G if k == 0 else min(k, G))
        out = torch.empty(max(1, m), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
        if m:
            self.ctx.check(self.ctx.L.igx_groupby_sort(self.h, arr, len(ts), m, ptr(out)))
        return out[:m]

    def topk_counts(self):
        """igx_groupby_topk_counts (synchronous): (top-Ks answered by the hinted path, by the full
        selection) so far."""
        out = (C.c_uint64 * 2)()
        self.ctx.check(self.ctx.L.igx_groupby_topk_counts(self.h, out))
        return int(out[0]), int(out[1])

    def gather(self, slots):
        """Packed rows (len(slots), key_bytes + 8*naggs + 8) for the given slots."""
        torch = torch_mod()
        row = self.fin["key_bytes"] + 8 * self.naggs + 8
        k = slots.numel()
        out = torch.empty((max(1, k), row), dtype=torch.uint8, device=slots.device)
        if k:
            self.ctx.check(self.ctx.L.igx_groupby_gather(self.h, ptr(slots), k, ptr(out)))
        return out[:k]

    def select_ge(self, agg, threshold, cap, sync=True):
        """igx_groupby_select_ge: the finalized interval's group slots whose aggregate `agg`
        (wrapped to its out_width, as gather wraps it) is >= threshold, in no particular order.
        Returns (slots, count): count is how many qualify; at most cap slots are listed, so
        count > cap means the list is incomplete.  sync=True reads the count (one host read) and
        returns slots[:min(count, cap)] and an int; sync=False returns the cap-entry tensor and
        the count as a device u64 tensor."""
        torch = torch_mod()
        ctx = self.ctx
        ctx.bind_stream()
        dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
        cnt = torch.empty(1, dtype=torch.uint64, device=dev)
        ctx.check(ctx.L.igx_groupby_select_ge(self.h, agg, threshold, ptr(out), cap, ptr(cnt)))
        if not sync:
            return out[:cap], cnt
        n = int(cnt.item())
        return out[:min(n, cap)], n

    def lookup(self, key_rows):
        """igx_groupby_lookup: key_rows is a device uint8 tensor (n, >= key_bytes) whose rows
        start with a packed key (rows from gather() can be passed as they are).  Returns (rows,
        found): rows (n, key_bytes + 8*naggs + 8) as gather() gives them for the keys that are
        groups of the finalized interval, zero rows for the others; found (n,) uint8."""
        torch = torch_mod()
        ctx = self.ctx
        ctx.bind_stream()
        kb = sum((w + 3) // 4 * 4 for w in self.key_widths)
        if key_rows.dim() != 2 or key_rows.dtype != torch.uint8 or key_rows.shape[1] < kb:
            raise ValueError(f"lookup: key_rows must be uint8 (n, >= {kb})")
        if key_rows.shape[0] and (key_rows.stride(1) != 1 or key_rows.stride(0) % 4 or key_rows.data_ptr() % 4):
            key_rows = key_rows[:, :kb].contiguous()   # the C ABI wants 4-byte aligned keys and stride
        n = key_rows.shape[0]
        row = kb + 8 * self.naggs + 8
        out = torch.empty((max(1, n), row), dtype=torch.uint8, device=key_rows.device)
        found = torch.empty(max(1, n), dtype=torch.uint8, device=key_rows.device)
        if n:
            ctx.check(ctx.L.igx_groupby_lookup(self.h, ptr(key_rows), key_rows.stride(0), n, ptr(out), ptr(found)))
        return out[:n], found[:n]

    def partition(self, nparts, out_widths=None):
        """igx_partition_groups: the finalized table's groups as packed rows (key | aggregates
        wrapped to out_widths | first index), grouped by owner part (FNV-1a over the key words
        mod nparts, as igx_partition_rows), stable in slot order within a part -- the sender
        side of the owner exchange, with the group count read on the device (works after
        finalize(sync=False)).  Returns (rows (capacity, row_bytes) u8, counts (nparts,) i64),
        both on the device; rows past the counts' sum are unused.  A table that lists more groups
        than its capacity (an over-capacity interval whose IGX_ENOSPC was not collected yet) gives
        -1 in every count: the rows are truncated (dist.exchange_partitioned raises on them)."""
        torch = torch_mod()
        ctx = self.ctx
        ctx.bind_stream()
        fin = self.fin
        rb = fin["key_bytes"] + 8 * self.naggs + 8
        dev = torch.device("cuda", torch.cuda.current_device())
        buf = getattr(self, "_part_buf", None)
        if buf is None or buf.shape != (self.capacity, rb):
            buf = self._part_buf = torch.empty((max(1, self.capacity), rb), dtype=torch.uint8, device=dev)
        cnt = torch.empty(nparts, dtype=torch.int64, device=dev)
        ow = (C.c_uint32 * max(1, self.naggs))(*(out_widths or self.out_widths))
        ctx.check(ctx.L.igx_partition_groups(ctx.h, C.byref(self._view), ow, nparts, ptr(buf), self.capacity,
                                             ptr(cnt)))
        return buf, cnt

    def destroy(self):
        if self.h:
            self.ctx.L.igx_groupby_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def table_tensors(tab, fin):
    """Dense copies of the finalized groups (occupied-slot order) as torch tensors:
    keys (G, key_bytes) u8, aggs [ (G,) u64 ], first (G,) u64."""
    torch = torch_mod()
    ctx = tab.ctx
    dev = torch.device("cuda", torch.cuda.current_device())
    G = fin["n_groups"]
    slots = torch.empty(max(1, G), dtype=torch.int32, device=dev)[:G]
    if G:
        ctx.check(ctx.L.igx_memcpy_d2d(ctx.h, ptr(slots), C.c_void_p(fin["groups_ptr"]), G * 4))
    rows = tab.gather(slots)
    kb = fin["key_bytes"]
    keys = rows[:, :kb].contiguous()
    # flat copies: a one-row slice counts as contiguous and keeps its byte offset and row
    # stride, which a u64 view rejects
    aggs = [rows[:, kb + 8 * i: kb + 8 * i + 8].reshape(-1).clone().view(torch.uint64)
            for i in range(tab.naggs)]
    first = rows[:, kb + 8 * tab.naggs:].reshape(-1).clone().view(torch.uint64)
    return keys, aggs, first


# ------------------------------------------------------------------------------------
# advise network-policy
# ------------------------------------------------------------------------------------
def np_mark(typ, pkt, hostip, raddr):
    """igx_np_mark: u8 keep mask of the advisor's event filter (advisor.go:279-292)."""
    torch = torch_mod()
    ctx = context()
    n = typ.numel()
    keep = torch.empty(max(4, (n + 3) // 4 * 4), dtype=torch.uint8, device=typ.device)
    ctx.check(ctx.L.igx_np_mark(ctx.h, ptr(typ), ptr(pkt), ptr(hostip), ptr(raddr), n, ptr(keep)))
    return keep[:n]


# ------------------------------------------------------------------------------------
# log2 histograms
# ------------------------------------------------------------------------------------
def hist_log2(dev, cont, delta, devs, ncont, divisor=1000, nslots=27, hist=None):
    torch = torch_mod()
    ctx = context()
    n = delta.numel()
    if hist is None:
        hist = torch.zeros((max(1, len(devs)) * ncont, nslots), dtype=torch.uint32, device=delta.device)
    hd = (C.c_uint32 * max(1, len(devs)))(*devs)
    ctx.check(ctx.L.igx_hist_log2(ctx.h, ptr(dev), ptr(cont), ptr(delta), n, hd, len(devs),
                                  ncont, divisor, nslots, ptr(hist)))
    return hist


def hist_log2_keyed(delta, cmd_flags=None, dev=None, divisor=1000, nslots=27, capacity=1 << 16):
    """biolatency with targ_per_flag / targ_per_disk (biolatency.bpf.c:116-150): one log2
    histogram per distinct raw hist_key{cmd_flags, dev}, any values (a column left None is the
    key field the BPF program leaves 0).  igx_log2_slots gives each event its slot, then a
    group-by on (cmd_flags, dev, slot) counts them (u32 slots, wrapping like the BPF map's).
    Returns [(cmd_flags, dev, u32 slots (nslots,))] in the order of each key's first event (the
    BPF map's own order is its hash order)."""
    import numpy as np
    from .columns import host
    torch = torch_mod()
    ctx = context()
    n = delta.numel()
    slot = torch.empty(max(4, (n + 3) // 4 * 4), dtype=torch.uint8, device=delta.device)[:n]
    keep = torch.empty(max(4, (n + 3) // 4 * 4), dtype=torch.uint8, device=delta.device)[:n]
    if n:
        ctx.check(ctx.L.igx_log2_slots(ctx.h, ptr(delta), n, divisor, nslots, ptr(slot), ptr(keep)))
    cols, widths = [], []
    for c in (cmd_flags, dev):
        if c is not None:
            cols.append(c)
            widths.append(4)
    cols.append(slot)
    widths.append(1)
    tab = Table(widths, [Agg(_abi.AGG_COUNT, 0, _abi.NO_COL, 4, 0)], capacity)
    try:
        if n:
            tab.update(cols, list(range(len(cols))), n, valid=keep)
        fin = tab.finalize()
        keys, aggs, first = table_tensors(tab, fin)
    finally:
        tab.destroy()
    k, cnt, f = host(keys), host(aggs[0]), host(first)
    nk = len(widths) - 1
    w = k[:, :4 * nk].copy().view(np.uint32).reshape(len(k), nk) if nk else np.zeros((len(k), 0), np.uint32)
    sl = k[:, 4 * nk]
    out = {}
    for i in range(len(k)):
        vals = [int(x) for x in w[i]]
        cf = vals.pop(0) if cmd_flags is not None else 0
        dv = vals.pop(0) if dev is not None else 0
        e = out.setdefault((cf, dv), [np.zeros(nslots, np.uint32), int(f[i])])
        e[0][sl[i]] = np.uint32(int(cnt[i]) & 0xFFFFFFFF)
        e[1] = min(e[1], int(f[i]))
    return [(cf, dv, h) for (cf, dv), (h, _) in sorted(out.items(), key=lambda kv: kv[1][1])]


# ------------------------------------------------------------------------------------
# block-I/O request pairing
# ------------------------------------------------------------------------------------
def req_join_tile():
    """igx_req_join_tile: rows per tile of the join's device scan (host call, no GPU)."""
    return int(_abi.lib().igx_req_join_tile())


def req_join(req, kind, ts, valid=None, pend_cap=None, sync=True):
    """igx_req_join: the start / issue / done join of block-I/O probe rows by request pointer
    (biotop.bpf.c:41-130, biolatency.bpf.c:47-154; the contract is in include/igx.h).
    req, ts: u64 (or int64) device tensors, kind and valid: uint8, all of n rows in stream order.
    Returns a dict: done, issue, who (int32 row ids; who is -1, i.e. IGX_NO_COL, without a START
    entry), delta (uint64, ts[done] - ts[issue] mod 2^64), one entry per emitting DONE in stream
    order; pend, the START / ISSUE rows still live at the end, in stream order (at most pend_cap
    of them, default n); n_done and n_pend, the true counts.  sync=True reads the counts (one
    host read) and trims the tensors; sync=False returns full-capacity tensors and the counts as
    device u64 tensors."""
    torch = torch_mod()
    ctx = context()
    n = int(req.numel())
    cap = n if pend_cap is None else int(pend_cap)
    dev = req.device
    req, kind, ts = req.contiguous(), kind.contiguous(), ts.contiguous()
    valid = None if valid is None else valid.contiguous()
    m = max(1, n)
    done, issue, who = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(3))
    delta = torch.empty(m, dtype=torch.uint64, device=dev)
    pend = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
    cnt = torch.empty(2, dtype=torch.uint64, device=dev)
    ctx.check(ctx.L.igx_req_join(ctx.h, ptr(req), ptr(kind), ptr(ts), ptr(valid), n, ptr(done), ptr(issue),
                                 ptr(who), ptr(delta), C.c_void_p(cnt.data_ptr()), ptr(pend), cap,
                                 C.c_void_p(cnt.data_ptr() + 8)))
    out = {"done": done[:n], "issue": issue[:n], "who": who[:n], "delta": delta[:n], "pend": pend[:cap],
           "n_done": cnt[0:1], "n_pend": cnt[1:2]}
    if not sync:
        return out
    nd, npend = (int(x) for x in cnt.cpu().view(torch.int64))
    for k in ("done", "issue", "who", "delta"):
        out[k] = out[k][:nd]
    out["pend"] = out["pend"][:min(npend, cap)]
    out["n_done"], out["n_pend"] = nd, npend
    return out


# ------------------------------------------------------------------------------------
# the two-register last-writer join (kprobe / kretprobe pairs keyed by the thread)
# ------------------------------------------------------------------------------------
def lw_join_tile():
    """igx_lw_join_tile: rows per tile of the join's device scan (host call, no GPU)."""
    return int(_abi.lib().igx_lw_join_tile())


def lw_join(key, kind, valid=None, pend_cap=None, sync=True):
    """igx_lw_join: the last-writer join with two registers per key (capable.bpf.c:87-248; the
    contract is in include/igx.h).  key: u64 (or int64) device tensor, kind (_abi.LW_*) and valid:
    uint8, all of n rows in stream order.
    Returns a dict: take, a, b (int32 row ids; b is -1, i.e. IGX_NO_COL, with B empty), one entry
    per emitting TAKE_A in stream order; pend, the rows still held in a register at the end, in
    stream order (at most pend_cap of them, default n); n_take and n_pend, the true counts.
    sync=True reads the counts (one host read) and trims the tensors; sync=False returns
    full-capacity tensors and the counts as device u64 tensors."""
    torch = torch_mod()
    ctx = context()
    n = int(key.numel())
    cap = n if pend_cap is None else int(pend_cap)
    dev = key.device
    key, kind = key.contiguous(), kind.contiguous()
    valid = None if valid is None else valid.contiguous()
    m = max(1, n)
    take_, a, b = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(3))
    pend = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
    cnt = torch.empty(2, dtype=torch.uint64, device=dev)
    ctx.check(ctx.L.igx_lw_join(ctx.h, ptr(key), ptr(kind), ptr(valid), n, ptr(take_), ptr(a), ptr(b),
                                C.c_void_p(cnt.data_ptr()), ptr(pend), cap, C.c_void_p(cnt.data_ptr() + 8)))
    out = {"take": take_[:n], "a": a[:n], "b": b[:n], "pend": pend[:cap], "n_take": cnt[0:1], "n_pend": cnt[1:2]}
    if not sync:
        return out
    nt, npend = (int(x) for x in cnt.cpu().view(torch.int64))
    for k in ("take", "a", "b"):
        out[k] = out[k][:nt]
    out["pend"] = out["pend"][:min(npend, cap)]
    out["n_take"], out["n_pend"] = nt, npend
    return out


# ------------------------------------------------------------------------------------
# the chained join through two maps, and trace tcp's per-row rules
# ------------------------------------------------------------------------------------
def chain_join_tile():
    """igx_chain_join_tile: rows per tile of the join's device scans (host call, no GPU)."""
    return int(_abi.lib().igx_chain_join_tile())


def chain_join(key1, key2, kind, valid=None, pend_cap=None, sync=True):
    """igx_chain_join: the join through two chained maps (tcptracer.bpf.c:52-64, :168-227,
    :296-330; the contract is in include/igx.h).  key1, key2: u64 (or int64) device tensors, kind
    (_abi.CJ_*) and valid: uint8, all of n rows in stream order.
    Returns a dict: take, pass (int32 row ids), one entry per emitting TAKE in stream order; pend,
    the ENTER / PASS / HELD rows still in a map at the end, in stream order (at most pend_cap of
    them, default n); n_take and n_pend, the true counts.  sync=True reads the counts (one host
    read) and trims the tensors; sync=False returns full-capacity tensors and the counts as
    device u64 tensors."""
    torch = torch_mod()
    ctx = context()
    n = int(key1.numel())
    if int(key2.numel()) != n or int(kind.numel()) != n:
        raise ValueError("chain_join: key1, key2 and kind must have the same number of rows")
    cap = n if pend_cap is None else int(pend_cap)
    dev = key1.device
    key1, key2, kind = key1.contiguous(), key2.contiguous(), kind.contiguous()
    valid = None if valid is None else valid.contiguous()
    m = max(1, n)
    take_, pass_ = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(2))
    pend = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
    cnt = torch.empty(2, dtype=torch.uint64, device=dev)
    ctx.check(ctx.L.igx_chain_join(ctx.h, ptr(key1), ptr(key2), ptr(kind), ptr(valid), n, ptr(take_), ptr(pass_),
                                   C.c_void_p(cnt.data_ptr()), ptr(pend), cap, C.c_void_p(cnt.data_ptr() + 8)))
    out = {"take": take_[:n], "pass": pass_[:n], "pend": pend[:cap], "n_take": cnt[0:1], "n_pend": cnt[1:2]}
    if not sync:
        return out
    nt, npend = (int(x) for x in cnt.cpu().view(torch.int64))
    for k in ("take", "pass"):
        out[k] = out[k][:nt]
    out["pend"] = out["pend"][:min(npend, cap)]
    out["n_take"], out["n_pend"] = nt, npend
    return out


TCP_ROW_FIELDS = ("probe", "tid", "pid", "uid", "mntns", "ret", "state", "family", "netns", "saddr", "daddr",
                  "dport", "sport", "num")
_TCP_ROW_BYTES = {"probe": 1, "tid": 4, "pid": 4, "uid": 4, "mntns": 8, "ret": 4, "state": 1, "family": 2,
                  "netns": 4, "saddr": 16, "daddr": 16, "dport": 2, "sport": 2, "num": 2}


def tcp_classify(rows, filter_pid=0, filter_uid=-1, mntns_set=None):
    """igx_tcp_classify: what each probe of trace tcp decides per row (tcptracer.bpf.c:79-166 and
    the probes; the contract is in include/igx.h).  rows: a dict of device tensors named as
    TCP_ROW_FIELDS (saddr / daddr are (n, 16) uint8; the others 1-D of their width).  mntns_set:
    None (no mount-namespace filter) or a device u64 tensor of up to 1024 ids sorted ascending.
    Returns a dict: tuple (uint8 (n, 40)), kind (uint8, _abi.CJ_* or _abi.TCP_NO_KIND), event
    (uint8, _abi.TCP_EV_*), key1 (int64, the thread).  Asynchronous."""
    torch = torch_mod()
    ctx = context()
    n = int(rows["probe"].numel())
    cols = {}
    for f in TCP_ROW_FIELDS:
        t = rows[f].contiguous()
        if t.numel() * t.element_size() != n * _TCP_ROW_BYTES[f]:
            raise ValueError(f"tcp_classify: column {f} must hold {_TCP_ROW_BYTES[f]} bytes per row")
        cols[f] = t
    dev = cols["probe"].device
    m = max(1, n)
    tup = torch.empty((m, _abi.TCP_TUPLE_BYTES // 8), dtype=torch.int64, device=dev).view(torch.uint8)
    kind, event = (torch.empty(m, dtype=torch.uint8, device=dev) for _ in range(2))
    key1 = torch.empty(m, dtype=torch.int64, device=dev)
    st = _abi.TcpRows(*[ptr(cols[f]) for f in TCP_ROW_FIELDS])
    ns = None if mntns_set is None else mntns_set.contiguous()
    ctx.check(ctx.L.igx_tcp_classify(ctx.h, C.byref(st), n, int(filter_pid) & 0xFFFFFFFF,
                                     int(filter_uid) & 0xFFFFFFFF, None if ns is None else C.c_void_p(ns.data_ptr()),
                                     0 if ns is None else int(ns.numel()), ptr(tup), ptr(kind), ptr(event),
                                     ptr(key1)))
    return {"tuple": tup[:n], "kind": kind[:n], "event": event[:n], "key1": key1[:n]}


# ------------------------------------------------------------------------------------
# traceloop: the enter / exit / cont join by timestamp
# ------------------------------------------------------------------------------------
TRACELOOP_NR_X86_64 = (60, 231, 15)    # exit, exit_group, rt_sigreturn (traceloop.bpf.c:12-35)
TRACELOOP_NR_ARM64 = (93, 94, 139)


def traceloop_tile():
    """igx_traceloop_tile: positions per tile of the join's device scan (host call, no GPU)."""
    return int(_abi.lib().igx_traceloop_tile())


def traceloop_join(mono_ts, sort_ts, typ, id, pid, valid=None, mntns=None, c_mono_ts=None, c_index=None,
                   c_valid=None, c_mntns=None, nr=TRACELOOP_NR_X86_64, sync=True):
    """igx_traceloop_join: traceloop's join of sys_enter, sys_exit and cont records by monotonic
    timestamp (tracer.go:246-545; the contract is in include/igx.h).  Syscall rows: mono_ts,
    sort_ts (u64 or int64), typ (uint8), id (uint16 or int16), pid (uint32 or int32), valid (uint8)
    and mntns (None: one container); cont rows: c_mono_ts, c_index (uint8), c_valid, c_mntns (given
    iff mntns is).  nr: the numbers of exit, exit_group and rt_sigreturn.
    Returns a dict: row, exit (int32 syscall rows; exit is -1, i.e. IGX_NO_COL, without an exit
    row), cls (uint8: 0 complete, 1 incomplete enter, 2 incomplete exit), cont ((n, 6) int32 cont
    rows, -1 for none), one entry per event in output order, and n_events.  sync=True reads the
    count (one host read) and trims the tensors; sync=False returns full-capacity tensors and
    the count as a device u64 tensor."""
    torch = torch_mod()
    ctx = context()
    ns = int(mono_ts.numel())
    nc = 0 if c_mono_ts is None else int(c_mono_ts.numel())
    dev = mono_ts.device
    cont = lambda t: None if t is None else t.contiguous()   # noqa: E731
    mono_ts, sort_ts, typ, id, pid, valid, mntns = (cont(t) for t in (mono_ts, sort_ts, typ, id, pid, valid, mntns))
    c_mono_ts, c_index, c_valid, c_mntns = (cont(t) for t in (c_mono_ts, c_index, c_valid, c_mntns))
    m = max(1, ns)
    row, ex = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(2))
    cls = torch.empty(m, dtype=torch.uint8, device=dev)
    ev_cont = torch.empty((m, 6), dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.uint64, device=dev)
    ctx.check(ctx.L.igx_traceloop_join(ctx.h, ptr(mntns), ptr(mono_ts), ptr(sort_ts), ptr(typ), ptr(id), ptr(pid),
                                       ptr(valid), ns, ptr(c_mntns), ptr(c_mono_ts), ptr(c_index), ptr(c_valid), nc,
                                       int(nr[0]), int(nr[1]), int(nr[2]), ptr(row), ptr(ex), ptr(cls), ptr(ev_cont),
                                       C.c_void_p(cnt.data_ptr())))
    out = {"row": row[:ns], "exit": ex[:ns], "cls": cls[:ns], "cont": ev_cont[:ns], "n_events": cnt}
    if not sync:
        return out
    nev = int(cnt.cpu().view(torch.int64)[0])
    for k in ("row", "exit", "cls", "cont"):
        out[k] = out[k][:nev]
    out["n_events"] = nev
    return out


# ------------------------------------------------------------------------------------
# profile cpu: row interning, kernel symbol lookup
# ------------------------------------------------------------------------------------
def _row_view(rows, row_bytes):
    """(pointer, stride in bytes, n) of a 2-D device tensor whose rows hold row_bytes bytes."""
    if rows.dim() != 2 or rows.shape[1] * rows.element_size() != row_bytes:
        raise ValueError(f"rows must be (n, {row_bytes} bytes)")
    if rows.shape[0] > 1 and rows.stride(1) != 1:
        rows = rows.contiguous()
    stride = rows.stride(0) * rows.element_size() if rows.shape[0] > 1 else row_bytes
    return rows, stride, int(rows.shape[0])


class Interner:
    """igx_intern: fixed-width rows of up to 1 KiB -> u32 ids by first appearance in the stream
    (what bpf_get_stackid and the stack map do for profile cpu; the contract is in
    include/igx.h).  rows are 2-D device tensors of row_bytes bytes per row (a row stride larger
    than that is passed through)."""

    def __init__(self, row_bytes, capacity, ctx=None):
        self.ctx = context() if ctx is None else ctx
        h = C.c_void_p()
        self.ctx.check(self.ctx.L.igx_intern_create(self.ctx.h, row_bytes, capacity, C.byref(h)))
        self.h = h
        self.row_bytes, self.capacity = row_bytes, capacity

    def add(self, rows, valid=None, first=False):
        """igx_intern_add (asynchronous): int32 ids of the rows (-1, i.e. IGX_NO_COL, where
        valid is 0).  first=True (igx_intern_add_first) returns (ids, first): first is uint8, 1
        where the row is the first valid occurrence of its content over all calls."""
        torch = torch_mod()
        self.ctx.bind_stream()
        rows, stride, n = _row_view(rows, self.row_bytes)
        valid = None if valid is None else valid.contiguous()
        out = torch.empty(max(1, n), dtype=torch.int32, device=rows.device)
        if not first:
            self.ctx.check(self.ctx.L.igx_intern_add(self.h, ptr(rows), stride, ptr(valid), n, ptr(out)))
            return out[:n]
        mask = torch.empty(max(1, n), dtype=torch.uint8, device=rows.device)
        self.ctx.check(self.ctx.L.igx_intern_add_first(self.h, ptr(rows), stride, ptr(valid), n, ptr(out), ptr(mask)))
        return out[:n], mask[:n]

    def count(self):
        """igx_intern_count (synchronises): distinct rows stored; IgxError(IGX_ENOSPC) once the
        capacity has overflowed."""
        n = C.c_uint64()
        self.ctx.check(self.ctx.L.igx_intern_count(self.h, C.byref(n)))
        return n.value

    def slots(self):
        """igx_intern_slots (host): S."""
        n = C.c_uint64()
        self.ctx.check(self.ctx.L.igx_intern_slots(self.h, C.byref(n)))
        return n.value

    def rows(self, ids):
        """igx_intern_rows (asynchronous): uint8 (k, row_bytes), the content of each id; zero
        rows for IGX_NO_COL and ids at or above the distinct count."""
        torch = torch_mod()
        self.ctx.bind_stream()
        if ids.dtype not in (torch.int32, torch.uint32):
            ids = ids.to(torch.int32)
        ids = ids.contiguous()
        k = int(ids.numel())
        out = torch.empty((max(1, k), self.row_bytes), dtype=torch.uint8, device=ids.device)
        self.ctx.check(self.ctx.L.igx_intern_rows(self.h, ptr(ids), k, ptr(out)))
        return out[:k]

    def destroy(self):
        if self.h:
            self.ctx.L.igx_intern_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def intern_hash_rows(rows, row_bytes=None, row_stride=None):
    """igx_intern_hash_rows (host, no GPU): the interner's 64-bit row hash of a C-contiguous
    numpy array of rows (row_bytes defaults to the row's bytes, row_stride to the array's)."""
    import numpy as np
    rows = np.ascontiguousarray(rows)
    if rows.ndim != 2:
        raise ValueError("rows must be 2-D")
    stride = rows.strides[0] if row_stride is None else row_stride
    rb = rows.shape[1] * rows.itemsize if row_bytes is None else row_bytes
    out = np.empty(rows.shape[0], np.uint64)
    rc = _abi.lib().igx_intern_hash_rows(rows.ctypes.data_as(C.c_void_p), rb, stride, rows.shape[0],
                                          out.ctypes.data_as(C.c_void_p))
    if rc:
        raise IgxError(rc, "igx_intern_hash_rows: bad row_bytes / row_stride")
    return out


def ksym_lookup(sym_addr, ips):
    """igx_ksym_lookup: findKernelSymbol (profile/cpu/tracer/tracer.go:184-208) of every
    address of ips (u64 device tensor, any shape) over the table sym_addr (u64 device tensor, in
    the order given).  Returns int32 symbol indices of ips' shape, -1 (IGX_NO_COL) for
    "[unknown]"."""
    torch = torch_mod()
    ctx = context()
    ips = ips.contiguous()
    sym_addr = sym_addr.contiguous()
    n = int(ips.numel())
    out = torch.empty(max(1, n), dtype=torch.int32, device=ips.device)
    ctx.check(ctx.L.igx_ksym_lookup(ctx.h, ptr(sym_addr), int(sym_addr.numel()), ptr(ips), n, ptr(out)))
    return out[:n].reshape(ips.shape)


# ------------------------------------------------------------------------------------
# advise seccomp-profile: per-mntns syscall sets
# ------------------------------------------------------------------------------------
class SeccompMap:
    """igx_seccomp: the syscalls_per_mntns map of advise seccomp-profile (the contract is in
    include/igx.h).  Columns are device tensors; namespaces for peek / delete are host ints."""

    def __init__(self, capacity=1024, nr_prctl=157, nr_seccomp=317, ctx=None):
        self.ctx = context() if ctx is None else ctx
        h = C.c_void_p()
        self.ctx.check(self.ctx.L.igx_seccomp_create(self.ctx.h, capacity, nr_prctl, nr_seccomp, C.byref(h)))
        self.h = h
        self.capacity = capacity

    def update(self, mntns, id, arg0, comm, compat=None, valid=None):
        """igx_seccomp_update (asynchronous).  mntns, arg0: 8-byte, id: 4-byte, compat, valid: 1-byte
        integer tensors of n rows; comm: (n, w) uint8 with w >= 4 (a row stride larger than w is
        passed through)."""
        self.ctx.bind_stream()
        n = int(mntns.numel())
        if comm.dim() != 2 or comm.element_size() != 1 or comm.shape[0] != n:
            raise ValueError("comm must be (n, width) bytes")
        if n > 1 and comm.stride(1) != 1:
            comm = comm.contiguous()
        stride = comm.stride(0) if n > 1 else comm.shape[1]
        cols = [mntns, id, arg0, compat, valid]
        for t, size in zip(cols, (8, 4, 8, 1, 1)):
            if t is not None and (t.element_size() != size or t.numel() != n):
                raise ValueError("column of the wrong width or length")
        mntns, id, arg0, compat, valid = (None if t is None else t.contiguous() for t in cols)
        self.ctx.check(self.ctx.L.igx_seccomp_update(self.h, ptr(mntns), ptr(id), ptr(arg0), ptr(comm), stride,
                                                     ptr(compat), ptr(valid), n))

    def _keys(self, mntns):
        import numpy as np
        torch = torch_mod()
        a = np.ascontiguousarray(np.asarray(mntns, dtype=np.uint64).reshape(-1))
        return torch.from_numpy(a.view(np.int64)).to(f"cuda:{self.ctx.device}"), a.size

    def peek(self, mntns):
        """igx_seccomp_peek: (values, found) as numpy uint8 arrays of (n, 501) and (n,)."""
        torch = torch_mod()
        self.ctx.bind_stream()
        keys, n = self._keys(mntns)
        out = torch.empty((max(1, n), _abi.SECCOMP_VALUE_BYTES), dtype=torch.uint8, device=keys.device)
        found = torch.empty(max(1, n), dtype=torch.uint8, device=keys.device)
        self.ctx.check(self.ctx.L.igx_seccomp_peek(self.h, ptr(keys), n, ptr(out), ptr(found)))
        return out[:n].cpu().numpy(), found[:n].cpu().numpy()

    def delete(self, mntns):
        """igx_seccomp_delete (asynchronous)."""
        self.ctx.bind_stream()
        keys, n = self._keys(mntns)
        self.ctx.check(self.ctx.L.igx_seccomp_delete(self.h, ptr(keys), n))

    def list(self):
        """igx_seccomp_list (synchronises): the namespaces that have an entry, sorted."""
        import numpy as np
        torch = torch_mod()
        self.ctx.bind_stream()
        cap = 2 * self.capacity   # no more than S slots can be live
        out = torch.empty(cap, dtype=torch.int64, device=f"cuda:{self.ctx.device}")
        n = C.c_uint64()
        self.ctx.check(self.ctx.L.igx_seccomp_list(self.h, ptr(out), cap, C.byref(n)))
        return np.sort(out[:n.value].cpu().numpy().view(np.uint64))

    def count(self):
        """igx_seccomp_count (synchronises): entries; IgxError(IGX_ENOSPC) once the capacity has
        overflowed."""
        self.ctx.bind_stream()
        n = C.c_uint64()
        self.ctx.check(self.ctx.L.igx_seccomp_count(self.h, C.byref(n)))
        return n.value

    def slots(self):
        """igx_seccomp_slots (host): S."""
        n = C.c_uint64()
        self.ctx.check(self.ctx.L.igx_seccomp_slots(self.h, C.byref(n)))
        return n.value

    def destroy(self):
        if self.h:
            self.ctx.L.igx_seccomp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def seccomp_home(mntns, nslots):
    """igx_seccomp_home (host, no GPU): the slot a namespace's probe starts at among nslots."""
    h = C.c_uint64()
    rc = _abi.lib().igx_seccomp_home(mntns, nslots, C.byref(h))
    if rc:
        raise IgxError(rc, "igx_seccomp_home: nslots must be a power of two")
    return h.value


# ------------------------------------------------------------------------------------
# data movement either side of the path
# ------------------------------------------------------------------------------------
def partition_rows(rows, key_bytes, nparts):
    """igx_partition_rows: (n, row_bytes) uint8 device rows grouped by owner part
    (FNV-1a over the key words mod nparts), stable within a part.  Returns (rows, counts)
    with counts a host list."""
    torch = torch_mod()
    ctx = context()
    n, rb = rows.shape
    rows = rows.contiguous()
    out = torch.empty_like(rows)
    cnt = torch.zeros(nparts, dtype=torch.int64, device=rows.device)
    ctx.check(ctx.L.igx_partition_rows(ctx.h, ptr(rows), n, rb, key_bytes, nparts, ptr(out), ptr(cnt)))
    return out, cnt.cpu().tolist()


def ip_text(addr, family, n=None, rowmap=None):
    """igx_ip_text: IPStringFromBytes (helpers.go:111-120) of n rows on the device.
    addr: uint8 (n, 16) or a byte view with a row stride; family: u16 column (or a byte view
    whose first two bytes per row are the family).  Returns uint8 (n, IPTEXT_WIDTH),
    zero-padded texts."""
    torch = torch_mod()
    ctx = context()
    n = addr.shape[0] if n is None else n
    astride = addr.stride(0) * addr.element_size()
    fstride = family.stride(0) * family.element_size()
    out = torch.empty((max(1, n), _abi.IPTEXT_WIDTH), dtype=torch.uint8, device=addr.device)
    if n:
        ctx.check(ctx.L.igx_ip_text(ctx.h, ptr(addr), astride, ptr(family), fstride,
                                    None if rowmap is None else ptr(rowmap), n, ptr(out)))
    return out[:n]


def ingest_open_events(samples, n=None, sample_bytes=_abi.OPEN_SAMPLE_BYTES, boot_to_wall_ns=0):
    """igx_ingest_open_events: trace open perf samples (device uint8, n x sample_bytes) ->
    the Event columns of trace/open/tracer/tracer.go:182-208 (timestamp, pid, uid, mntns, ret,
    fd, err as int64 / u32 / u64 tensors; comm (n, 16) and path (n, 256) uint8)."""
    torch = torch_mod()
    ctx = context()
    n = samples.numel() // sample_bytes if n is None else n
    dev = samples.device
    m = max(1, n)
    cols = {"timestamp": torch.empty(m, dtype=torch.int64, device=dev),
            "pid": torch.empty(m, dtype=torch.uint32, device=dev),
            "uid": torch.empty(m, dtype=torch.uint32, device=dev),
            "mntns": torch.empty(m, dtype=torch.uint64, device=dev),
            "ret": torch.empty(m, dtype=torch.int64, device=dev),
            "fd": torch.empty(m, dtype=torch.int64, device=dev),
            "err": torch.empty(m, dtype=torch.int64, device=dev),
            "comm": torch.empty((m, 16), dtype=torch.uint8, device=dev),
            "path": torch.empty((m, 256), dtype=torch.uint8, device=dev)}
    oc = _abi.OpenCols(*[cols[f].data_ptr() for f, _ in _abi.OpenCols._fields_])
    ctx.check(ctx.L.igx_ingest_open_events(ctx.h, ptr(samples), n, sample_bytes, boot_to_wall_ns, C.byref(oc)))
    return {k: v[:n] for k, v in cols.items()}


def ingest_aos(records, n, rec_bytes, fields, device=None):
    """igx_ingest_aos: records (device uint8, n x rec_bytes) -> {name: SoA column}.
    fields: [(name, offset, width, dtype)] with dtype a torch dtype (width 1/2/4/8) or
    None for a byte column (n, width)."""
    torch = torch_mod()
    ctx = context()
    dev = records.device if device is None else device
    cols = {}
    for name, off, width, dt in fields:
        cols[name] = (torch.empty((n, width), dtype=torch.uint8, device=dev) if dt is None
                      else torch.empty(n, dtype=dt, device=dev))
    offs = (C.c_uint32 * len(fields))(*[f[1] for f in fields])
    wids = (C.c_uint32 * len(fields))(*[f[2] for f in fields])
    outs = (C.c_void_p * len(fields))(*[cols[f[0]].data_ptr() for f in fields])
    ctx.check(ctx.L.igx_ingest_aos(ctx.h, ptr(records), n, rec_bytes, offs, wids, len(fields), outs))
    return cols
