"""The aggregation gadgets as their tracers expose them: top tcp / file / block-io,
profile block-io / cpu, advise seccomp-profile, traceloop, trace capabilities and trace tcp, on
top of libigx.so.

Each `Top*` class is the user-space half of a reference tracer plus the BPF map update it
drains, re-cut for batches of events resident in HBM:

  feed(events)   the BPF probe for every event of a batch: the probe's filters (fused
                 group-by predicates), the map key, lookup-or-insert and the `+=` updates
                 (igx_groupby_update_ex on the device)
  nextStats()    tracer.nextStats: one Stats row per map entry, top.SortStats(SortBy),
                 then the map is emptied for the next interval (the deferred Delete loop)
  NextEvent()    one tick of tracer.run: nextStats() truncated to MaxRows, wrapped in
                 top.Event (the eventCallback payload)

References (paths under the reference root):
  top tcp       pkg/gadgets/top/tcp/tracer/tracer.go:147-265, bpf/tcptop.bpf.c:33-110,
                types/types.go:27-101
  top file      pkg/gadgets/top/file/tracer/tracer.go:148-247, bpf/filetop.bpf.c:39-94,
                types/types.go:30-62
  top block-io  pkg/gadgets/top/block-io/tracer/tracer.go:211-310, bpf/biotop.bpf.c:85-130,
                types/types.go:31-65
  profile block-io  pkg/gadgets/profile/block-io/tracer/tracer.go:56-90 (getReport),
                tracer/gadget.go:85-143 (reportToString), bpf/biolatency.bpf.c:100-154
  profile cpu   pkg/gadgets/profile/cpu/tracer/bpf/profile.bpf.c:60-114, tracer/tracer.go:86-322,
                types/types.go:27-56
  trace capabilities  pkg/gadgets/trace/capabilities/tracer/bpf/capable.bpf.c:87-248,
                tracer/tracer.go:224-318, types/types.go:35-73
  trace tcp     pkg/gadgets/trace/tcp/tracer/bpf/tcptracer.bpf.c:79-372, tracer/tracer.go:198-234,
                types/types.go:22-55

The reference's pre-sort order (BPF hash iteration) is replaced by each group's first
event index; everything else -- keys, wrap widths, sort order including
the DESC tie reversal, truncation -- is the reference's.  Sorting runs on the device over
the whole table; only the rows that are returned are copied to the host.
"""
from __future__ import annotations

import bisect
import ipaddress
import json
from dataclasses import dataclass, field
from typing import Dict, List, Optional

from . import _abi, engine
from .columns import Columns, host
from .runtime import torch_mod
from . import sort as _sort
from . import top as _top

AF_INET, AF_INET6 = 2, 10                 # syscall.AF_INET / AF_INET6
REQ_OP_WRITE = 1                          # biotop.bpf.c:106 (REQ_OP_MASK = 0xff)

# ------------------------------------------------------------------------------------
# pkg/gadgets/helpers.go
# ------------------------------------------------------------------------------------


def FromCString(b) -> str:
    """helpers.go:76-83: bytes up to the first NUL."""
    b = bytes(b)
    i = b.find(b"\0")
    return (b if i < 0 else b[:i]).decode("utf-8", "replace")


def IPStringFromBytes(b, ipType: int) -> str:
    """helpers.go:111-120: netip.AddrFrom4 / AddrFrom16 .String()."""
    b = bytes(b)
    if ipType == 4:
        return ".".join(str(x) for x in b[:4])
    if ipType == 6:
        if b[:10] == b"\0" * 10 and b[10:12] == b"\xff\xff":   # netip prints 4in6 dotted
            return "::ffff:" + ".".join(str(x) for x in b[12:16])
        return str(ipaddress.IPv6Address(b))
    return ""


# ------------------------------------------------------------------------------------
# table-backed top gadget
# ------------------------------------------------------------------------------------
@dataclass
class Event:
    """top.Event[T] (pkg/gadgets/top/top.go:30-34)."""
    Error: str = ""
    Stats: list = field(default_factory=list)


def _pred(col, cmp, ref_bytes, negate=0, guard=None):
    """igx_pred; guard = (column, value bytes): the test applies only where that column
    holds that value (a check one probe makes and another does not)."""
    p = _abi.Pred()
    p.col, p.cmp, p.negate, p.ref_len = col, cmp, negate, len(ref_bytes)
    for i, x in enumerate(ref_bytes):
        p.ref[i] = x
    if guard is not None:
        p.guard_col, gref = guard
        p.guard_len = len(gref)
        for i, x in enumerate(gref):
            p.guard_ref[i] = x
    return p


class _TopTracer:
    """Shared machinery.  Subclasses define:
      EVENT      [(name, kind, width)] event columns the probe reads (SoA, device)
      KEY        names of the map key's fields, in key-struct order
      AGGS       [(kind, value column | None, cond column | None, cond value, out width, divisor)]
      STATS_COLS Columns of the Stats struct (what sortBy names refer to)
      SORT_SRC   Stats column -> ("agg", i) | ("key", field) | ("const",)
      ALIASES    [(name, event column, torch dtype)]: the column's memory read as another type
                 (appended after EVENT, e.g. an argument the probe declares signed)
      SortByDefault
    and _preds() (the probe's filters) and _stats(rows) (Stats objects)."""

    EVENT: list = []
    KEY: list = []
    AGGS: list = []
    SORT_SRC: Dict[str, tuple] = {}
    SortByDefault: list = []
    ALIASES: list = []

    def __init__(self, MaxRows=_top.MaxRowsDefault, SortBy=None, capacity=1 << 20, Interval=1, ctx=None):
        self.MaxRows = MaxRows
        self.SortBy = list(self.SortByDefault if SortBy is None else SortBy)
        self.Interval = Interval
        self.ev_index = {name: i for i, (name, _, _) in enumerate(self.EVENT)}
        for j, (name, _, _) in enumerate(self.ALIASES):
            self.ev_index[name] = len(self.EVENT) + j
        self.ev_width = {name: w for name, _, w in self.EVENT}
        widths = [self.ev_width[k] for k in self.KEY]
        aggs = []
        for kind, vcol, ccol, cval, ow, div in self.AGGS:
            aggs.append(_abi.Agg(kind, 0 if vcol is None else self.ev_index[vcol],
                                 _abi.NO_COL if ccol is None else self.ev_index[ccol], ow, cval, div))
        self.table = engine.Table(widths, aggs, capacity, ctx=ctx)
        self.key_off = {}
        o = 0
        for k in self.KEY:
            self.key_off[k] = o
            o += (self.ev_width[k] + 3) // 4 * 4
        self.key_bytes = o
        self.batches = []          # (base_idx, n, events) fed this interval
        self.next_idx = 0

    # -- the probe --------------------------------------------------------------------
    def _preds(self):
        return []

    def feed(self, events: dict, n: Optional[int] = None, base_idx: Optional[int] = None):
        """Run the BPF probe over a batch: events maps EVENT names to device tensors."""
        torch = torch_mod()
        n = int(events[self.KEY[0]].shape[0]) if n is None else n
        base = self.next_idx if base_idx is None else base_idx
        cols = []
        for name, kind, w in self.EVENT:
            t = events.get(name)
            if t is None:
                # columns the probe does not need for this config (e.g. a condition column
                # that no aggregate uses) still need a readable pointer
                t = torch.zeros(max(1, n), dtype=torch.uint8, device=events[self.KEY[0]].device)
            cols.append(t)
        for _, src, dtype in self.ALIASES:
            cols.append(cols[self.ev_index[src]].view(getattr(torch, dtype)))
        self.table.update(cols, [self.ev_index[k] for k in self.KEY], n, base, self._preds())
        self.batches.append((base, n, events))
        self.next_idx = base + n

    # -- nextStats ----------------------------------------------------------------------
    def _sort_keys(self, sort_by):
        """top.SortStats(stats, sortBy, colMap) as table sort keys (sort.Prepare rules:
        unknown / virtual columns dropped; bool columns skipped at sort time)."""
        keys = []
        for sk in _sort._prepare_raw(self.STATS_COLS, sort_by):
            if sk.kind in (_abi.KIND_BOOL, _abi.KIND_OTHER):
                continue
            name = self.STATS_COLS.GetOrderedColumns()[sk.col].Name.lower()
            src = self.SORT_SRC.get(name)
            if src is None:
                raise _abi.IgxError(_abi.IGX_ENOTSUP, f"sorting by {name!r} needs the host")
            desc = bool(sk.desc)
            if src[0] == "agg":
                keys.append((_abi.TSRC_AGG, src[1], desc))
            elif src[0] == "iptext":      # Saddr / Daddr: IPStringFromBytes text order
                keys.append((_abi.TSRC_IPTEXT, (self.key_off[src[1]], self.key_off[src[2]]), desc))
            elif src[0] == "key":
                f = src[1]
                kind = src[2] if len(src) > 2 else sk.kind
                keys.append((_abi.TSRC_KEY, (self.key_off[f], self.ev_width[f], kind), desc))
            else:
                keys.append((_abi.TSRC_CONST, 0, desc))
        return keys

    def _gather_first(self, first, name):
        """Values of event column `name` at global event indices `first` (the BPF first
        insert's attributes: filetop.bpf.c:68-85)."""
        torch = torch_mod()
        out = [None] * len(first)
        bases = [b for b, _, _ in self.batches]
        by_batch = {}
        for i, f in enumerate(first):
            j = bisect.bisect_right(bases, int(f)) - 1
            by_batch.setdefault(j, []).append((i, int(f) - bases[j]))
        for j, lst in by_batch.items():
            t = self.batches[j][2].get(name)
            if t is None:
                continue
            li = torch.tensor([r for _, r in lst], dtype=torch.int32, device=t.device)
            vals = host(_take(t, li))
            for (i, _), v in zip(lst, vals):
                out[i] = v
        return out

    def nextStats(self, limit: Optional[int] = None):
        """All Stats of the interval in SortStats order (limit: only the first `limit`
        rows are materialised -- the order is the same); empties the map."""
        fin = self.table.finalize()
        G = fin["n_groups"]
        k = G if limit is None else min(limit, G)
        stats = []
        if k:
            slots = self.table.sort(self._sort_keys(self.SortBy), k)
            rows = host(self.table.gather(slots))
            stats = self._stats(rows)
        self.table.reset()
        self.batches = []
        return stats

    def NextEvent(self):
        """One tick of tracer.run: stats[:MaxRows] in a top.Event."""
        return Event(Stats=self.nextStats(limit=self.MaxRows))

    def _unpack(self, rows):
        """Packed table rows -> (dict of key fields as numpy, aggregates list, first)."""
        import numpy as np
        kf = {}
        np_t = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
        for f in self.KEY:
            o, w = self.key_off[f], self.ev_width[f]
            seg = np.ascontiguousarray(rows[:, o:o + w])
            kf[f] = seg if w not in np_t else seg.view(np_t[w]).ravel()
        kb = self.key_bytes
        aggs = [np.ascontiguousarray(rows[:, kb + 8 * i:kb + 8 * i + 8]).view(np.uint64).ravel()
                for i in range(len(self.AGGS))]
        first = np.ascontiguousarray(rows[:, kb + 8 * len(self.AGGS):]).view(np.uint64).ravel()
        return kf, aggs, first

    def destroy(self):
        self.table.destroy()


def _take(t, li):
    from . import engine                     # igx_take on the device
    return engine.take([t], li)[0]


def _stats_columns(fields, extractors=(), virtual=()):
    cols = Columns([("node", "string", 64), ("namespace", "string", 64), ("pod", "string", 64),
                    ("container", "string", 64), ("mntns", "uint64")] + list(fields))
    for name in extractors:
        cols.SetExtractor(name, lambda s: "")
    for name in virtual:
        cols.AddColumn(name, lambda s: "")
    return cols


_ENRICH = {"node": ("const",), "namespace": ("const",), "pod": ("const",), "container": ("const",)}

# ------------------------------------------------------------------------------------
# top tcp
# ------------------------------------------------------------------------------------


@dataclass
class TcpStats:
    """pkg/gadgets/top/tcp/types/types.go:46-58."""
    Node: str = ""           # eventtypes.CommonData (pkg/types/types.go:73-87), filled by enrichers
    Namespace: str = ""
    Pod: str = ""
    Container: str = ""
    MountNsID: int = 0
    Pid: int = 0
    Comm: str = ""
    Family: int = 0
    Saddr: str = ""
    Daddr: str = ""
    Sport: int = 0
    Dport: int = 0
    Sent: int = 0
    Received: int = 0
    FirstIndex: int = 0      # canonical pre-sort position (not in the reference struct)


def copied_pred(copied_col, dir_col):
    """ig_toptcp_clean's `if (copied <= 0) return 0;` (tcptop.bpf.c:124-130) as a group-by
    predicate: `copied > 0` (int32) on the rows with dir == 1 (tcp_cleanup_rbuf); sends pass."""
    return _pred(copied_col, _abi.CMP_GT, (0).to_bytes(4, "little"), guard=(dir_col, b"\x01"))


class TopTcpTracer(_TopTracer):
    """top tcp: probe_ip keyed by ip_key_t, sent/received += size."""
    EVENT = [("saddr", "bytes", 16), ("daddr", "bytes", 16), ("mntns", "uint", 8), ("pid", "uint", 4),
             ("comm", "bytes", 16), ("lport", "uint", 2), ("dport", "uint", 2), ("family", "uint", 2),
             ("size", "uint", 4), ("dir", "uint", 1)]
    KEY = ["saddr", "daddr", "mntns", "pid", "comm", "lport", "dport", "family"]
    # dir 0 = tcp_sendmsg (sent), 1 = tcp_cleanup_rbuf (received)
    AGGS = [(_abi.AGG_SUM, "size", "dir", 0, 8, 0), (_abi.AGG_SUM, "size", "dir", 1, 8, 0)]
    # the receive probe's argument is `int copied` (tcptop.bpf.c:125)
    ALIASES = [("copied", "size", "int32")]
    STATS_COLS = _stats_columns([("pid", "int32"), ("comm", "string", 16), ("ip", "uint16"),
                                 ("saddr", "string", 46), ("daddr", "string", 46), ("sport", "uint16"),
                                 ("dport", "uint16"), ("sent", "uint64"), ("recv", "uint64")],
                                extractors=("ip", "sent", "recv"), virtual=("local", "remote"))
    SORT_SRC = dict(_ENRICH, mntns=("key", "mntns"), pid=("key", "pid", _abi.KIND_INT),
                    comm=("key", "comm"), ip=("key", "family"), sport=("key", "lport"),
                    dport=("key", "dport"), sent=("agg", 0), recv=("agg", 1),
                    saddr=("iptext", "saddr", "family"), daddr=("iptext", "daddr", "family"))
    SortByDefault = ["-sent", "-recv"]      # types.go:27

    def __init__(self, TargetPid=0, TargetFamily=-1, **kw):
        super().__init__(**kw)
        self.TargetPid = TargetPid
        self.TargetFamily = TargetFamily

    def _preds(self):
        """tcptop.bpf.c:42-55: target_pid (0 = all), target_family (-1 = all), then the
        probe drops every family but AF_INET / AF_INET6; before any of it the receive probe
        returns when `copied <= 0` (tcptop.bpf.c:124-130; sends have no such check)."""
        fam, pid = self.ev_index["family"], self.ev_index["pid"]
        recv_pos = copied_pred(self.ev_index["copied"], self.ev_index["dir"])
        inet = _pred(fam, _abi.CMP_IN, AF_INET.to_bytes(2, "little") + AF_INET6.to_bytes(2, "little"))
        if self.TargetFamily not in (-1, AF_INET, AF_INET6):
            # an impossible family: the two tests contradict, no event is kept
            return [_pred(fam, _abi.CMP_EQ, (self.TargetFamily & 0xFFFF).to_bytes(2, "little")), inet]
        preds = [inet if self.TargetFamily == -1 else
                 _pred(fam, _abi.CMP_EQ, self.TargetFamily.to_bytes(2, "little")), recv_pos]
        if self.TargetPid:
            preds.append(_pred(pid, _abi.CMP_EQ, (self.TargetPid & 0xFFFFFFFF).to_bytes(4, "little")))
        return preds

    def _stats(self, rows):
        kf, (sent, recv), first = self._unpack(rows)
        out = []
        for i in range(rows.shape[0]):
            fam = int(kf["family"][i])
            ipt = 6 if fam == AF_INET6 else 4           # tracer.go:199-203
            pid = int(kf["pid"][i])
            out.append(TcpStats(MountNsID=int(kf["mntns"][i]), Pid=pid - (1 << 32) if pid >= 1 << 31 else pid,
                                Comm=FromCString(kf["comm"][i]), Family=fam,
                                Saddr=IPStringFromBytes(kf["saddr"][i], ipt),
                                Daddr=IPStringFromBytes(kf["daddr"][i], ipt),
                                Sport=int(kf["lport"][i]), Dport=int(kf["dport"][i]),
                                Sent=int(sent[i]), Received=int(recv[i]), FirstIndex=int(first[i])))
        return out


# ------------------------------------------------------------------------------------
# top file
# ------------------------------------------------------------------------------------
@dataclass
class FileStats:
    """pkg/gadgets/top/file/types/types.go:37-51."""
    Node: str = ""           # eventtypes.CommonData (pkg/types/types.go:73-87), filled by enrichers
    Namespace: str = ""
    Pod: str = ""
    Container: str = ""
    MountNsID: int = 0
    Pid: int = 0
    Tid: int = 0
    Comm: str = ""
    Reads: int = 0
    Writes: int = 0
    ReadBytes: int = 0
    WriteBytes: int = 0
    FileType: int = 0
    Filename: str = ""
    FirstIndex: int = 0


READ, WRITE = 0, 1                       # filetop.h enum op


class TopFileTracer(_TopTracer):
    """top file: probe_entry keyed by file_id{inode, dev, pid, tid}; reads/writes++ and
    read/write_bytes += count; the first insert records mntns / comm / filename / type,
    which here are the attributes of the group's first event."""
    EVENT = [("inode", "uint", 8), ("dev", "uint", 4), ("pid", "uint", 4), ("tid", "uint", 4),
             ("op", "uint", 1), ("count", "uint", 4), ("ftype", "uint", 1)]
    KEY = ["inode", "dev", "pid", "tid"]
    AGGS = [(_abi.AGG_COUNT, None, "op", READ, 8, 0), (_abi.AGG_SUM, "count", "op", READ, 8, 0),
            (_abi.AGG_COUNT, None, "op", WRITE, 8, 0), (_abi.AGG_SUM, "count", "op", WRITE, 8, 0)]
    STATS_COLS = _stats_columns([("pid", "uint32"), ("tid", "uint32"), ("comm", "string", 16),
                                 ("reads", "uint64"), ("writes", "uint64"), ("rbytes", "uint64"),
                                 ("wbytes", "uint64"), ("t", "uint8"), ("file", "string", 64)],
                                extractors=("rbytes", "wbytes"))
    SORT_SRC = dict(_ENRICH, pid=("key", "pid"), tid=("key", "tid"), reads=("agg", 0),
                    rbytes=("agg", 1), writes=("agg", 2), wbytes=("agg", 3))
    SortByDefault = ["-reads", "-writes", "-rbytes", "-wbytes"]   # types.go:30

    def __init__(self, TargetPid=0, AllFiles=False, **kw):
        super().__init__(**kw)
        self.TargetPid = TargetPid
        self.AllFiles = AllFiles

    def _preds(self):
        """filetop.bpf.c:49-60: target_pid; regular_file_only && !S_ISREG -> drop (the
        event's ftype is the BPF type_ letter: 'R' regular, 'S' socket, 'O' other)."""
        preds = []
        if self.TargetPid:
            preds.append(_pred(self.ev_index["pid"], _abi.CMP_EQ, (self.TargetPid & 0xFFFFFFFF).to_bytes(4, "little")))
        if not self.AllFiles:
            preds.append(_pred(self.ev_index["ftype"], _abi.CMP_EQ, b"R"))
        return preds

    def _stats(self, rows):
        kf, (reads, rbytes, writes, wbytes), first = self._unpack(rows)
        mntns = self._gather_first(first, "mntns")
        comm = self._gather_first(first, "comm")
        fname = self._gather_first(first, "filename")
        ftype = self._gather_first(first, "ftype")
        out = []
        for i in range(rows.shape[0]):
            out.append(FileStats(MountNsID=int(mntns[i]) if mntns[i] is not None else 0,
                                 Pid=int(kf["pid"][i]), Tid=int(kf["tid"][i]),
                                 Comm=FromCString(comm[i].tobytes()) if comm[i] is not None else "",
                                 Reads=int(reads[i]), Writes=int(writes[i]), ReadBytes=int(rbytes[i]),
                                 WriteBytes=int(wbytes[i]),
                                 FileType=int(ftype[i]) if ftype[i] is not None else 0,
                                 Filename=FromCString(fname[i].tobytes()) if fname[i] is not None else "",
                                 FirstIndex=int(first[i])))
        return out


# ------------------------------------------------------------------------------------
# top block-io
# ------------------------------------------------------------------------------------
@dataclass
class BlockIOStats:
    """pkg/gadgets/top/block-io/types/types.go:35-48."""
    Node: str = ""           # eventtypes.CommonData (pkg/types/types.go:73-87), filled by enrichers
    Namespace: str = ""
    Pod: str = ""
    Container: str = ""
    MountNsID: int = 0
    Pid: int = 0
    Comm: str = ""
    Write: bool = False
    Major: int = 0
    Minor: int = 0
    Bytes: int = 0
    MicroSecs: int = 0
    Operations: int = 0
    FirstIndex: int = 0


class TopBlockIOTracer(_TopTracer):
    """top block-io: ig_topio_done keyed by info_t{mntnsid, pid, rwflag, major, minor,
    name}; us += (now - start)/1000, bytes += data_len, io++ (u32)."""
    EVENT = [("mntns", "uint", 8), ("pid", "uint", 4), ("rwflag", "int", 4), ("major", "int", 4),
             ("minor", "int", 4), ("comm", "bytes", 16), ("data_len", "uint", 8), ("delta_ns", "uint", 8)]
    KEY = ["mntns", "pid", "rwflag", "major", "minor", "comm"]
    AGGS = [(_abi.AGG_SUM, "data_len", None, 0, 8, 0), (_abi.AGG_SUM, "delta_ns", None, 0, 8, 1000),
            (_abi.AGG_COUNT, None, None, 0, 4, 0)]
    STATS_COLS = _stats_columns([("pid", "int32"), ("comm", "string", 16), ("r/w", "bool"),
                                 ("major", "int"), ("minor", "int"), ("bytes", "uint64"),
                                 ("time", "uint64"), ("ops", "uint32")], extractors=("r/w",))
    SORT_SRC = dict(_ENRICH, mntns=("key", "mntns"), pid=("key", "pid", _abi.KIND_INT),
                    comm=("key", "comm"), major=("key", "major", _abi.KIND_INT),
                    minor=("key", "minor", _abi.KIND_INT), bytes=("agg", 0), time=("agg", 1),
                    ops=("agg", 2))
    SortByDefault = ["-ops", "-bytes", "-time"]    # types.go:31

    def _stats(self, rows):
        import numpy as np
        kf, (nbytes, us, io), first = self._unpack(rows)
        out = []
        for i in range(rows.shape[0]):
            pid = int(kf["pid"][i])
            out.append(BlockIOStats(MountNsID=int(kf["mntns"][i]), Pid=pid - (1 << 32) if pid >= 1 << 31 else pid,
                                    Comm=FromCString(kf["comm"][i]), Write=int(kf["rwflag"][i]) != 0,
                                    Major=int(np.int32(np.uint32(kf["major"][i]))),
                                    Minor=int(np.int32(np.uint32(kf["minor"][i]))),
                                    Bytes=int(nbytes[i]), MicroSecs=int(us[i]),
                                    Operations=int(io[i]) & 0xFFFFFFFF, FirstIndex=int(first[i])))
        return out


# ------------------------------------------------------------------------------------
# output side: the Stats types' column tags and JSON fields
# ------------------------------------------------------------------------------------
# eventtypes.CommonData + WithMountNsID (pkg/types/types.go:73-87,217-219)
_COMMON_COLS = [("Node", "string", "node,template:node", ["kubernetes"]),
                ("Namespace", "string", "namespace,template:namespace", ["kubernetes"]),
                ("Pod", "string", "pod,template:pod", ["kubernetes"]),
                ("Container", "string", "container,template:container", ["kubernetes", "runtime"]),
                ("MountNsID", "uint64", "mntns,template:ns", [])]
_COMMON_JSON = [("Node", "node", True), ("Namespace", "namespace", True), ("Pod", "pod", True),
                ("Container", "container", True), ("MountNsID", "mountnsid", True)]

STATS_OUTPUT = {
    # pkg/gadgets/top/tcp/types/types.go:46-101
    "tcp": {
        "fields": _COMMON_COLS + [("Pid", "int32", "pid,template:pid", []), ("Comm", "string", "comm,template:comm", []),
                                  ("Family", "uint16", "ip,maxWidth:2", []),
                                  ("Saddr", "string", "saddr,template:ipaddr,hide", []),
                                  ("Daddr", "string", "daddr,template:ipaddr,hide", []),
                                  ("Sport", "uint16", "sport,template:ipport,hide", []),
                                  ("Dport", "uint16", "dport,template:ipport,hide", []),
                                  ("Sent", "uint64", "sent,order:1002", []),
                                  ("Received", "uint64", "recv,order:1003", [])],
        "json": _COMMON_JSON + [("Pid", "pid", True), ("Comm", "comm", True), ("Family", "family", True),
                                ("Saddr", "saddr", True), ("Daddr", "daddr", True), ("Sport", "sport", True),
                                ("Dport", "dport", True), ("Sent", "sent", True), ("Received", "received", True)],
    },
    # pkg/gadgets/top/file/types/types.go:37-66
    "file": {
        "fields": _COMMON_COLS + [("Pid", "uint32", "pid,template:pid", []), ("Tid", "uint32", "tid,template:pid,hide", []),
                                  ("Comm", "string", "comm,template:comm", []), ("Reads", "uint64", "reads", []),
                                  ("Writes", "uint64", "writes", []), ("ReadBytes", "uint64", "rbytes", []),
                                  ("WriteBytes", "uint64", "wbytes", []), ("FileType", "uint8", "T,maxWidth:1", []),
                                  ("Filename", "string", "file", [])],
        "json": _COMMON_JSON + [("Pid", "pid", True), ("Tid", "tid", True), ("Comm", "comm", True),
                                ("Reads", "reads", True), ("Writes", "writes", True), ("ReadBytes", "rbytes", True),
                                ("WriteBytes", "wbytes", True), ("FileType", "fileType", True),
                                ("Filename", "filename", True)],
    },
    # pkg/gadgets/top/block-io/types/types.go:34-61
    "block-io": {
        "fields": _COMMON_COLS + [("Pid", "int32", "pid", []), ("Comm", "string", "comm", []),
                                  ("Write", "bool", "r/w,maxWidth:3", []), ("Major", "int", "major", []),
                                  ("Minor", "int", "minor", []), ("Bytes", "uint64", "bytes", []),
                                  ("MicroSecs", "uint64", "time", []), ("Operations", "uint32", "ops", [])],
        "json": _COMMON_JSON + [("Pid", "pid", True), ("Comm", "comm", True), ("Write", "write", True),
                                ("Major", "major", True), ("Minor", "minor", True), ("Bytes", "bytes", True),
                                ("MicroSecs", "us", True), ("Operations", "ops", True)],
    },
}


def StatsColumns(gadget: str):
    """types.GetColumns() of a top gadget's Stats: the tagged fields plus its extractors and
    virtual columns, as a textcolumns.ColumnMap (every column; see OutputColumns for the
    frontends' tag filter)."""
    from . import textcolumns as T
    spec = STATS_OUTPUT[gadget]
    cm = T.ColumnMap([(attr, kind, tag) for attr, kind, tag, _ in spec["fields"]])
    for attr, kind, tag, tags in spec["fields"]:
        cm.cols[tag.split(",")[0].lower()].Tags = list(tags)
    if gadget == "tcp":
        cm.SetExtractor("ip", lambda st: "4" if st.Family == AF_INET else "6")
        cm.SetExtractor("sent", lambda st: T.BytesSize(float(st.Sent)))
        cm.SetExtractor("recv", lambda st: T.BytesSize(float(st.Received)))
        cm.AddColumn("local", lambda st: f"{st.Saddr}:{st.Sport}", MinWidth=21, MaxWidth=51, Order=1000)
        cm.AddColumn("remote", lambda st: f"{st.Daddr}:{st.Dport}", MinWidth=21, MaxWidth=51, Order=1000)
    elif gadget == "file":
        cm.SetExtractor("rbytes", lambda st: T.BytesSize(float(st.ReadBytes)))
        cm.SetExtractor("wbytes", lambda st: T.BytesSize(float(st.WriteBytes)))
        cm.SetExtractor("T", lambda st: chr(st.FileType))
    else:
        cm.SetExtractor("r/w", lambda st: "W" if st.Write else "R")
    return cm


def OutputColumns(gadget: str, metadata_tag: str = ""):
    """The column map a frontend formats with (parser-tableformatter.go:60-65): columns
    without tags, plus those carrying metadata_tag ("kubernetes" for kubectl-gadget, "runtime"
    for ig with a container runtime; "" = untagged only)."""
    cm = StatsColumns(gadget)
    cm.cols = {k: c for k, c in cm.cols.items() if not c.Tags or (metadata_tag and metadata_tag in c.Tags)}
    return cm


def render_table(gadget: str, stats, metadata_tag: str = "", terminal_width: int = 0, columns=None) -> str:
    """The columns output of one interval (GadgetParser.TransformIntoTable over the interval's
    []*Stats, cmd/common/utils/parser-tableformatter.go:106-111)."""
    from . import textcolumns as T
    f = T.TextColumnsFormatter(OutputColumns(gadget, metadata_tag), DefaultColumns=columns)
    return T.TransformIntoTable(f, stats, terminal_width)


def render_json(gadget: str, stats) -> str:
    """-o json: json.Marshal of the interval's []*Stats (cmd/common/registry.go:511-520)."""
    from . import textcolumns as T
    return T.marshal_array(stats, STATS_OUTPUT[gadget]["json"])


def rwflag_of(cmd_flags):
    """biotop.bpf.c:106: !!((cmd_flags & REQ_OP_MASK) == REQ_OP_WRITE) (host helper)."""
    return int((int(cmd_flags) & 0xFF) == REQ_OP_WRITE)


def _cat_rows(a, b):
    """Rows of a, then rows of b (same dtype and row shape).  Unsigned columns are joined
    through the signed view of the same width."""
    torch = torch_mod()
    if a is None or a.shape[0] == 0:
        return b
    signed = {torch.uint16: torch.int16, torch.uint32: torch.int32, torch.uint64: torch.int64}.get(b.dtype)
    if signed is None:
        return torch.cat([a, b])
    return torch.cat([a.contiguous().view(signed), b.contiguous().view(signed)]).view(b.dtype)


class _ReqCarry:
    """The in-band state of the request pairing (include/igx.h, igx_req_join): the START /
    ISSUE rows still live after a batch, every column, put in front of the next batch -- what
    the reference keeps in its `start` / `whobyreq` maps between probes."""

    def __init__(self, pending_cap):
        self.pending_cap = pending_cap
        self.rows = None          # {column: tensor} of the carried rows, in stream order

    def join(self, cols):
        """cols: {name: device tensor} with req, kind, ts and whatever travels with a row.
        Returns (all rows with the carry in front, the join's result); keeps the new carry."""
        if self.rows is not None:
            cols = {k: _cat_rows(self.rows[k], v) for k, v in cols.items()}
        j = engine.req_join(cols["req"], cols["kind"], cols["ts"], pend_cap=self.pending_cap)
        if j["n_pend"] > self.pending_cap:
            raise _abi.IgxError(_abi.IGX_ENOSPC, f"block-io pairing: {j['n_pend']} requests in flight exceed "
                                                 f"pending_cap={self.pending_cap}")
        names = list(cols)
        self.rows = dict(zip(names, engine.take([cols[k] for k in names], j["pend"])))
        return cols, j


class TopBlockIOProbeTracer(TopBlockIOTracer):
    """top block-io from its three probes' own rows: blk_account_io_start (kind START, whose
    mntns / pid / comm are who_t), blk_mq_start_request (ISSUE: ts, data_len) and
    blk_account_io_done (DONE: ts, cmd_flags, major, minor), paired by request pointer on the
    device (biotop.bpf.c:41-130) and then counted by TopBlockIOTracer's table unchanged.

    Requests still in flight after a batch are carried into the next one, across nextStats too:
    the reference's start / whobyreq maps live on while only counts is drained
    (tracer.go:211-282).  More than pending_cap of them raises IgxError(IGX_ENOSPC).  The carry
    belongs to the tracer, so StreamingTopTracer, which alternates between two tracers, would
    split it: feed one tracer."""

    PROBE = ("req", "kind", "ts", "mntns", "pid", "comm", "data_len", "cmd_flags", "major", "minor")

    def __init__(self, pending_cap=1 << 20, **kw):
        super().__init__(**kw)
        self._carry = _ReqCarry(pending_cap)

    def feed(self, events: dict, n: Optional[int] = None, base_idx: Optional[int] = None):
        """events maps PROBE names to device tensors of the batch's rows in stream order."""
        torch = torch_mod()
        n = int(events["req"].shape[0]) if n is None else n
        cols, j = self._carry.join({k: events[k][:n] for k in self.PROBE})
        nd = j["n_done"]
        if nd == 0:
            return
        mntns, pid, comm = engine.take([cols["mntns"], cols["pid"], cols["comm"]], j["who"], pad=True)
        data_len, = engine.take([cols["data_len"]], j["issue"])
        cmd_flags, major, minor = engine.take([cols["cmd_flags"], cols["major"], cols["minor"]], j["done"])
        # rwflag_of per row (biotop.bpf.c:108)
        rwflag = ((cmd_flags.view(torch.int32) & 0xFF) == REQ_OP_WRITE).to(torch.int32)
        super().feed({"mntns": mntns, "pid": pid, "rwflag": rwflag, "major": major, "minor": minor, "comm": comm,
                      "data_len": data_len, "delta_ns": j["delta"]}, nd, base_idx)

    @property
    def pending(self):
        """Requests in flight (rows carried into the next batch)."""
        return 0 if self._carry.rows is None else int(self._carry.rows["req"].shape[0])


# ------------------------------------------------------------------------------------
# streaming interval mode
# ------------------------------------------------------------------------------------
class StreamingTopTracer:
    """The top tracers' run loop (e.g. pkg/gadgets/top/tcp/tracer/tracer.go:228-265: a
    ticker calls nextStats, emits stats[:MaxRows], counts Iterations down) over two device
    tables.  A tick swaps the tables before draining, so the next interval's events are
    aggregated into the other table -- on a HIP stream of its own -- while the host sorts,
    gathers and builds the Stats of the interval that just closed (the BPF map keeps taking
    events while nextStats walks and deletes it).

    cls: a _TopTracer subclass; kw: its constructor arguments (MaxRows, SortBy, capacity,
    filter options).  Events get global indices continuing across intervals."""

    def __init__(self, cls, Iterations=0, device=None, **kw):
        torch = torch_mod()
        from .runtime import Context
        dev = torch.cuda.current_device() if device is None else device
        self.Iterations = Iterations
        self.count = Iterations
        self.streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        self.ctxs = [Context(dev, stream=s) for s in self.streams]
        self.tracers = []
        for s, c in zip(self.streams, self.ctxs):
            with torch.cuda.stream(s):
                self.tracers.append(cls(ctx=c, **kw))
        self.cur = 0
        self.next_idx = 0
        self.done = False

    def feed(self, events: dict, n: Optional[int] = None):
        """Events of the current interval (device tensors made on torch's current stream)."""
        torch = torch_mod()
        tr, s = self.tracers[self.cur], self.streams[self.cur]
        s.wait_stream(torch.cuda.current_stream())
        n = int(events[tr.KEY[0]].shape[0]) if n is None else n
        with torch.cuda.stream(s):
            tr.feed(events, n, base_idx=self.next_idx)
        for t in events.values():
            t.record_stream(s)           # the caller's tensors stay alive for the update
        self.next_idx += n

    def tick(self):
        """ticker.C: the interval ends -> top.Event with stats[:MaxRows]; None after the
        last iteration."""
        if self.done:
            return None
        torch = torch_mod()
        closed = self.cur
        self.cur ^= 1                    # later feeds go to the other table
        with torch.cuda.stream(self.streams[closed]):
            ev = self.tracers[closed].NextEvent()
        if self.Iterations > 0:
            self.count -= 1
            self.done = self.count == 0
        return ev

    def run(self, intervals):
        """Generator over intervals (each an iterable of event batches): interval k+1's
        updates are enqueued before the host blocks on interval k's drain."""
        pending = False
        for batches in intervals:
            if pending:
                # enqueue this interval's batches into the fresh table, then drain the old one
                closed = self.cur ^ 1
                for b in batches:
                    self.feed(b)
                torch = torch_mod()
                with torch.cuda.stream(self.streams[closed]):
                    ev = self.tracers[closed].NextEvent()
                yield ev
                if self.Iterations > 0:
                    self.count -= 1
                    if self.count == 0:
                        return
            else:
                for b in batches:
                    self.feed(b)
            self.cur ^= 1
            pending = True
        if pending:
            yield self.tick_closed()

    def tick_closed(self):
        torch = torch_mod()
        closed = self.cur ^ 1
        with torch.cuda.stream(self.streams[closed]):
            return self.tracers[closed].NextEvent()

    def destroy(self):
        for t in self.tracers:
            t.destroy()
        for c in self.ctxs:
            c.close()



# ------------------------------------------------------------------------------------
# profile block-io
# ------------------------------------------------------------------------------------
MAX_SLOTS = 27          # biolatency.h:6


@dataclass
class Data:
    """profile/block-io/types/types.go:17-21."""
    count: int
    intervalStart: int
    intervalEnd: int


@dataclass
class Report:
    """profile/block-io/types/types.go:23-27."""
    ValType: str = ""
    Data: List[Data] = field(default_factory=list)
    Time: str = ""

    def to_json(self) -> str:
        """json.Marshal(report) with the reference's omitempty tags."""
        d = {}
        if self.ValType:
            d["valType"] = self.ValType
        if self.Data:
            d["data"] = [{k: v for k, v in (("count", x.count), ("intervalStart", x.intervalStart),
                                             ("intervalEnd", x.intervalEnd)) if k != "intervalEnd" or v}
                         for x in self.Data]
        if self.Time:
            d["ts"] = self.Time
        return json.dumps(d, separators=(",", ":"))


def getReport(slots, val_type="usecs") -> Report:
    """tracer.go:56-90: Data[i] = {Count, 1<<i, (1<<(i+1))-1}, truncated to
    data[:indexMax] -- the highest non-zero slot is dropped (reference behaviour)."""
    data, index_max = [], 0
    for i, v in enumerate(slots):
        v = int(v)
        if v > 0:
            index_max = i
        data.append(Data(v, (1 << (i + 1)) >> 1, (1 << (i + 1)) - 1))
    return Report(ValType=val_type, Data=data[:index_max])


def starsToString(val: int, valMax: int, width: int) -> str:
    """gadget.go:88-110 (bcc print_stars)."""
    if valMax == 0:
        return " " * width
    stars = min(val, valMax) * width // valMax
    s = "*" * stars + " " * (width - stars)
    if val > valMax:
        s += "+"
    return s


def reportToString(report: Report) -> str:
    """gadget.go:112-143 (bcc print_log2_hist)."""
    if not report.Data:
        return ""
    val_max = max(d.count for d in report.Data)
    out = ["%5s%-19s : count    distribution\n" % ("", report.ValType)]
    for d in report.Data:
        out.append("%10d -> %-10d : %-8d |%s|\n" % (d.intervalStart, d.intervalEnd, d.count,
                                                   starsToString(d.count, val_max, 40)))
    return "".join(out)


class ProfileBlockIOTracer:
    """profile block-io: ig_profio_done's log2 histogram on the device.

    devs=None is the shipped gadget (no targ_per_disk / targ_per_flag: one key {0,0} for
    every I/O); devs=[MKDEV(major, minor), ...] (and ncont > 1 with a container column)
    keys per device (and per container), the C3 extension.  ms=True is targ_ms."""

    def __init__(self, devs=None, ncont=1, ms=False, per_disk=False, per_flag=False):
        self.devs = list(devs or [])
        self.ncont = ncont
        self.divisor = 1000000 if ms else 1000
        self.val_type = "msecs" if ms else "usecs"
        self.hist = None
        # targ_per_disk / targ_per_flag (biolatency.bpf.c:116-131): histograms keyed by the raw
        # hist_key{cmd_flags, dev} values instead of the dense dev x container index
        self.per_disk, self.per_flag = per_disk, per_flag
        self.keyed = {}   # (cmd_flags, dev) -> u32 slots, in first-event order

    def feed(self, delta_ns, dev=None, cont=None, cmd_flags=None):
        if self.per_disk or self.per_flag:
            import numpy as np
            for cf, dv, h in engine.hist_log2_keyed(delta_ns, cmd_flags if self.per_flag else None,
                                                    dev if self.per_disk else None, self.divisor, MAX_SLOTS):
                cur = self.keyed.setdefault((cf, dv), np.zeros(MAX_SLOTS, np.uint32))
                cur += h   # u32 wrap, like __sync_fetch_and_add on the map's u32 slots
            return
        self.hist = engine.hist_log2(dev, cont, delta_ns, self.devs, self.ncont, self.divisor,
                                     MAX_SLOTS, hist=self.hist)

    def feed_probes(self, req, kind, ts, dev=None, cmd_flags=None, pending_cap=1 << 20):
        """The probes' own rows instead of finished latencies: block_rq_insert / block_rq_issue
        (kind ISSUE: ts) and block_rq_complete (DONE: ts, and the dev / cmd_flags the key is
        built from), paired by request pointer on the device (biolatency.bpf.c:47-154), then
        feed() with the latencies as s64 -- a negative one is dropped there, as the probe's
        `delta < 0` branch does (:115-117).  Requests in flight are carried to the next call."""
        torch = torch_mod()
        if getattr(self, "_carry", None) is None:
            self._carry = _ReqCarry(pending_cap)
        cols = {"req": req, "kind": kind, "ts": ts}
        if dev is not None:
            cols["dev"] = dev
        if cmd_flags is not None:
            cols["cmd_flags"] = cmd_flags
        cols, j = self._carry.join(cols)
        if j["n_done"] == 0:
            return
        at_done = dict(zip([k for k in ("dev", "cmd_flags") if k in cols],
                           engine.take([cols[k] for k in ("dev", "cmd_flags") if k in cols], j["done"])))
        self.feed(j["delta"].view(torch.int64), dev=at_done.get("dev"), cmd_flags=at_done.get("cmd_flags"))

    def slots(self):
        """u32 slots per key, host numpy (nkeys, 27); keyed mode: in first-event order."""
        import numpy as np
        if self.per_disk or self.per_flag:
            if not self.keyed:
                return np.zeros((0, MAX_SLOTS), np.uint32)
            return np.stack(list(self.keyed.values()))
        if self.hist is None:
            return np.zeros((max(1, len(self.devs)) * self.ncont, MAX_SLOTS), np.uint32)
        return host(self.hist)

    def keys(self):
        """keyed mode: the hist_key{cmd_flags, dev} of each row of slots()."""
        return list(self.keyed.keys())

    def getReport(self, key: int = 0) -> Report:
        """The reference reads the first key only (NextKey(nil), the BPF map's hash order); key
        picks one here (first-event order in keyed mode)."""
        return getReport(self.slots()[key], self.val_type)

    def Stop(self) -> str:
        """tracer.go:92-113: json.Marshal(getReport(...))."""
        return self.getReport().to_json()


# ------------------------------------------------------------------------------------
# profile cpu
# ------------------------------------------------------------------------------------
PERF_MAX_STACK_DEPTH = 127      # profile/cpu/tracer/tracer.go:57
UNKNOWN_SYMBOL = "[unknown]"    # tracer.go:207, :239


@dataclass
class CpuReport:
    """profile/cpu/types/types.go:27-37 (CommonData: pkg/types/types.go:73-87)."""
    Node: str = ""
    Namespace: str = ""
    Pod: str = ""
    Container: str = ""
    Comm: str = ""
    Pid: int = 0
    UserStack: List[str] = field(default_factory=list)
    KernelStack: List[str] = field(default_factory=list)
    Count: int = 0
    MntnsID: int = 0             # `json:"-"`
    FirstIndex: int = 0          # canonical pre-sort position (not in the reference struct)

    def ExtraLines(self) -> List[str]:
        """types.go:47-56: the kernel stack, then the user stack, innermost frame last."""
        return (["\t" + s for s in reversed(self.KernelStack)] +
                ["\t" + s for s in reversed(self.UserStack)])

    def to_json(self) -> str:
        """json.Marshal(report): every field is omitempty, and an empty slice is empty."""
        import dataclasses
        from . import textcolumns as T
        view = dataclasses.replace(self, UserStack=self.UserStack or None, KernelStack=self.KernelStack or None)
        return T.marshal(view, _CPU_JSON)


_CPU_JSON = _COMMON_JSON[:4] + [("Comm", "comm", True), ("Pid", "pid", True), ("UserStack", "userStack", True),
                                ("KernelStack", "kernelStack", True), ("Count", "count", True)]


def readKernelSymbols(text: str):
    """tracer.go:139-177 over the text of /proc/kallsyms: [(addr, name)] in file order.  Lines
    with fewer than three fields are skipped; a first field that strconv.ParseUint(s, 16, 64)
    rejects is an error."""
    out = []
    for line in text.splitlines():
        fields = line.split()
        if len(fields) < 3:
            continue
        a = fields[0]
        if any(c not in "0123456789abcdefABCDEF" for c in a) or int(a, 16) >> 64:
            raise ValueError(f'strconv.ParseUint: parsing "{a}": invalid syntax')
        out.append((int(a, 16), fields[2]))
    return out


class ProfileCpuTracer:
    """profile cpu: ig_prof_cpu (profile.bpf.c:60-114) over batches of samples, and
    collectResult (tracer.go:293-322).

    The stack map is an engine.Interner (one for kernel and user stacks, as one `stackmap`
    serves both bpf_get_stackid calls; kernel rows are added before user rows in each feed), the
    counts map a device table keyed by key_t (profile.h:9-16).  max_stacks and capacity bound
    the distinct stacks and keys (IgxError(IGX_ENOSPC) past them); the reference's max_entries
    and the stack map's -EEXIST are not modelled, nor is filter_by_mnt_ns.

    kallsyms: [(addr, name)] or the text of /proc/kallsyms (readKernelSymbols), in file order."""

    def __init__(self, user_stack_only=False, kernel_stack_only=False, include_idle=False,
                 depth=PERF_MAX_STACK_DEPTH, max_stacks=1 << 16, capacity=1 << 16, kallsyms=None, ctx=None):
        import numpy as np
        from .columns import to_device
        self.user_stack_only, self.kernel_stack_only = bool(user_stack_only), bool(kernel_stack_only)
        self.include_idle = bool(include_idle)
        self.depth = depth
        syms = readKernelSymbols(kallsyms) if isinstance(kallsyms, str) else list(kallsyms or [])
        self.sym_names = [name for _, name in syms]
        self.sym_addr = to_device(np.array([a for a, _ in syms], dtype=np.uint64))
        self.stacks = engine.Interner(depth * 8, max_stacks, ctx=ctx)
        # key_t: kernel_ip u64, mntns_id u64, pid u32, user_stack_id i32, kern_stack_id i32, name[16]
        self.table = engine.Table([8, 8, 4, 4, 4, 16], [_abi.Agg(_abi.AGG_COUNT, 0, _abi.NO_COL, 8, 0)], capacity,
                                  ctx=ctx)
        self.next_idx = 0

    def _stack_ids(self, off, keep, stack, status):
        """profile.bpf.c:90-98: -1 when the other side only was asked for, the error
        bpf_get_stackid returned, or the stack's id."""
        torch = torch_mod()
        if off:
            return torch.full_like(status, -1)
        ok = keep & (status >= 0)
        ids = self.stacks.add(stack.view(torch.uint8).reshape(stack.shape[0], -1), ok.to(torch.uint8))
        return torch.where(status < 0, status, ids)

    def feed(self, pid, tid, mntns, comm, ip, kstack, kstatus, ustack, ustatus):
        """One batch of samples as device columns: pid, tid u32; mntns, ip u64; comm (n, 16)
        uint8; kstack, ustack (n, depth) u64, zero-padded; kstatus, ustatus int32 (>= 0: the
        stack walk succeeded, < 0: the error bpf_get_stackid returned)."""
        torch = torch_mod()
        n = int(pid.shape[0])
        if n == 0:
            return
        keep = torch.ones(n, dtype=torch.bool, device=pid.device) if self.include_idle else \
            tid.view(torch.int32) != 0                                    # :72-73
        ks = self._stack_ids(self.user_stack_only, keep, kstack, kstatus.view(torch.int32))
        us = self._stack_ids(self.kernel_stack_only, keep, ustack, ustatus.view(torch.int32))
        ip64 = ip.view(torch.int64)
        kernel_ip = torch.where((ks >= 0) & (ip64 < 0), ip64, torch.zeros_like(ip64))   # :100-107
        cols = [kernel_ip.view(torch.uint64), mntns, pid, us, ks, comm]
        self.table.update(cols, list(range(6)), n, self.next_idx, valid=keep.to(torch.uint8))
        self.next_idx += n

    def reports(self) -> List[CpuReport]:
        """collectResult: one report per key, ascending count (ties: first occurrence)."""
        import numpy as np
        from .columns import to_device
        torch = torch_mod()
        self.stacks.count()          # IGX_ENOSPC if the stack map overflowed
        fin = self.table.finalize()
        G = fin["n_groups"]
        if not G:
            return []
        rows = host(self.table.gather(self.table.sort([(_abi.TSRC_AGG, 0, False)], G)))
        f = lambda o, dt: np.ascontiguousarray(rows[:, o:o + np.dtype(dt).itemsize]).view(dt).ravel()   # noqa: E731
        mntns, pid, us, ks = f(8, np.uint64), f(16, np.uint32), f(20, np.int32), f(24, np.int32)
        count, first = f(44, np.uint64), f(52, np.uint64)
        ustacks, kstacks = {}, {}
        uid = np.unique(us[us >= 0])
        if len(uid):
            st = host(self.stacks.rows(to_device(uid.astype(np.int32)))).view(np.uint64)
            for i, row in zip(uid, st):
                z = np.flatnonzero(row == 0)
                ustacks[int(i)] = [UNKNOWN_SYMBOL] * int(z[0] if len(z) else len(row))
        kid = np.unique(ks[ks >= 0])
        if len(kid):
            frames = self.stacks.rows(to_device(kid.astype(np.int32))).view(torch.uint64)
            idx = host(engine.ksym_lookup(self.sym_addr, frames))
            for i, row, sym in zip(kid, host(frames), idx):
                z = np.flatnonzero(row == 0)
                kstacks[int(i)] = [UNKNOWN_SYMBOL if j < 0 else self.sym_names[j]
                                   for j in sym[:int(z[0] if len(z) else len(row))]]
        return [CpuReport(Comm=FromCString(rows[i, 28:44]), Pid=int(pid[i]), UserStack=list(ustacks.get(int(us[i]), [])),
                          KernelStack=list(kstacks.get(int(ks[i]), [])), Count=int(count[i]), MntnsID=int(mntns[i]),
                          FirstIndex=int(first[i])) for i in range(G)]

    def Stop(self) -> str:
        """tracer.go:266-274, :321: json.Marshal([]Report)."""
        return "[" + ",".join(r.to_json() for r in self.reports()) + "]"

    def destroy(self):
        self.table.destroy()
        self.stacks.destroy()


# ------------------------------------------------------------------------------------
# advise seccomp-profile (pkg/gadgets/advise/seccomp/tracer/tracer.go, syscalls.go;
# pkg/gadget-collection/gadgets/advise/seccomp/syscalls.go, gadget.go:217-251)
# ------------------------------------------------------------------------------------
SYSCALLS_COUNT = _abi.SECCOMP_SYSCALLS
# (__NR_prctl, __NR_seccomp) per GOARCH (seccomp.bpf.c:20-51)
SECCOMP_NR = {"amd64": (157, 317), "arm64": (167, 277)}
_ARCHES = {   # tracer/syscalls.go:29-48
    "amd64": ["SCMP_ARCH_X86_64", "SCMP_ARCH_X86", "SCMP_ARCH_X32"],
    "arm64": ["SCMP_ARCH_ARM", "SCMP_ARCH_AARCH64"],
    "mips64": ["SCMP_ARCH_MIPS", "SCMP_ARCH_MIPS64", "SCMP_ARCH_MIPS64N32"],
    "mips64n32": ["SCMP_ARCH_MIPS", "SCMP_ARCH_MIPS64", "SCMP_ARCH_MIPS64N32"],
    "mipsel64": ["SCMP_ARCH_MIPSEL", "SCMP_ARCH_MIPSEL64", "SCMP_ARCH_MIPSEL64N32"],
    "mipsel64n32": ["SCMP_ARCH_MIPSEL", "SCMP_ARCH_MIPSEL64", "SCMP_ARCH_MIPSEL64N32"],
    "s390x": ["SCMP_ARCH_S390", "SCMP_ARCH_S390X"],
}


def go_marshal(v, indent: Optional[str] = None, sort_maps: bool = True, _depth: int = 0) -> str:
    """json.Marshal (indent None) or json.MarshalIndent(v, "", indent) of nested dicts, lists,
    strings, ints, bools and None.  A dict stands for a Go map when sort_maps (keys sorted as
    encoding/json sorts them) and for a struct otherwise (insertion order = field order)."""
    from . import textcolumns as T
    if isinstance(v, dict):
        items = sorted(v.items()) if sort_maps else list(v.items())
        parts = [T.go_json_string(k) + (":" if indent is None else ": ") + go_marshal(x, indent, sort_maps, _depth + 1)
                 for k, x in items]
        o, c = "{", "}"
    elif isinstance(v, (list, tuple)):
        parts = [go_marshal(x, indent, sort_maps, _depth + 1) for x in v]
        o, c = "[", "]"
    else:
        return T.go_json_value(v)
    if not parts:
        return o + c
    if indent is None:
        return o + ",".join(parts) + c
    pad = "\n" + indent * (_depth + 1)
    return o + pad + ("," + pad).join(parts) + "\n" + indent * _depth + c


def syscallArrToNameList(value, names=None) -> List[str]:
    """tracer.go:90-105: the names of the ids whose presence byte is set, sorted as sort.Strings
    sorts; "syscall%d" for an id the table does not name.  names: {id: name}, default the
    generated x86_64 table."""
    if names is None:
        from ._syscalls import X86_64 as names
    out = [names.get(i) or "syscall%d" % i for i, b in enumerate(bytes(value)[:SYSCALLS_COUNT]) if b]
    return sorted(out, key=lambda s: s.encode("utf-8", "surrogatepass"))


def Arches(goarch: str = "amd64") -> List[str]:
    """tracer/syscalls.go:29-48 for runtime.GOARCH == goarch."""
    return list(_ARCHES.get(goarch, []))


def SyscallNamesToLinuxSeccomp(syscallNames, goarch: str = "amd64") -> dict:
    """tracer/syscalls.go:50-65 as json.Marshal lays out specs.LinuxSeccomp (field order kept):
    the omitempty fields that are empty here -- args, flags, listener*, errno returns, and
    architectures on an unknown GOARCH -- are left out.  names: null for None, as a nil slice."""
    d = {"defaultAction": "SCMP_ACT_ERRNO"}
    if Arches(goarch):
        d["architectures"] = Arches(goarch)
    d["syscalls"] = [{"names": None if syscallNames is None else list(syscallNames), "action": "SCMP_ACT_ALLOW"}]
    return d


@dataclass
class SeccompProfileNsName:
    """gadget.go:206-215."""
    namespace: str = ""
    name: str = ""
    generateName: bool = False


def syscallNamesToSeccompPolicy(profileName: SeccompProfileNsName, syscallNames, goarch: str = "amd64") -> dict:
    """gadget-collection/gadgets/advise/seccomp/syscalls.go:27-62 as json.Marshal lays out the
    security-profiles-operator's SeccompProfile: empty omitempty fields are left out (the empty
    label and annotation maps too); creationTimestamp (a struct) and status stay."""
    meta = {}
    if profileName.generateName:
        meta["generateName"] = profileName.name + "-"
    elif profileName.name:
        meta["name"] = profileName.name
    if profileName.namespace:
        meta["namespace"] = profileName.namespace
    meta["creationTimestamp"] = None
    spec = {"defaultAction": "SCMP_ACT_ERRNO"}
    if Arches(goarch):
        spec["architectures"] = Arches(goarch)
    spec["syscalls"] = [{"names": None if syscallNames is None else list(syscallNames), "action": "SCMP_ACT_ALLOW"}]
    return {"metadata": meta, "spec": spec, "status": {}}


def _atoi(s: str):
    """strconv.Atoi: an optional sign and decimal digits within int64, else None."""
    body = s[1:] if s[:1] in ("+", "-") else s
    if not body or not all("0" <= ch <= "9" for ch in body):
        return None
    v = int(s)
    return v if -(1 << 63) <= v < (1 << 63) else None


def getSeccompProfileNextName(profileNames, podName: str) -> str:
    """gadget.go:217-251 over the names of the profile list.  strings.TrimLeft takes a cutset,
    not a prefix, and so does this."""
    counter = 0
    for name in profileNames:
        if not name.startswith(podName):
            continue
        if name == podName and counter == 0:
            counter += 1
            continue
        c = _atoi(name.lstrip(podName + "-"))
        if c is None:
            continue
        if c > counter:
            counter = c
    return podName if counter == 0 else "%s-%d" % (podName, counter + 1)


@dataclass(eq=False)
class SeccompContainer:
    """What the tracer reads of a containercollection.Container.  Compared by identity, as
    the reference's map is keyed by pointer."""
    Name: str
    Mntns: int


class AdviseSeccompTracer:
    """advise seccomp-profile: ig_seccomp_e (seccomp.bpf.c:67-139) over batches of sys_enter
    rows, and the Tracer of tracer.go:42-179.  The map is an engine.SeccompMap; capacity bounds
    the distinct mount namespaces it can ever hold (IgxError(IGX_ENOSPC) from Peek past it; the
    reference's max_entries is not modelled).  names: {id: name} for syscallArrToNameList."""

    def __init__(self, capacity=1024, goarch="amd64", names=None, ctx=None):
        nr_prctl, nr_seccomp = SECCOMP_NR[goarch]
        self.map = engine.SeccompMap(capacity, nr_prctl, nr_seccomp, ctx=ctx)
        self.names = names
        self.containers: Dict[object, Optional[List[str]]] = {}

    def feed(self, mntns, id, arg0, comm, compat=None):
        """One batch of sys_enter rows as device columns: mntns, arg0 u64; id u32; comm (n, 16)
        uint8; compat u8 (is_x86_compat; None where the architecture has none)."""
        self.map.update(mntns, id, arg0, comm, compat)

    def Peek(self, mntns: int) -> List[str]:
        """tracer.go:107-122; LookupError("no syscall found") for an absent entry."""
        value, found = self.map.peek([mntns])
        self.map.count()          # IGX_ENOSPC if the map overflowed
        if not found[0]:
            raise LookupError("no syscall found")   # the container just hasn't done any syscall
        return syscallArrToNameList(value[0], self.names)

    def Delete(self, mntns: int):
        self.map.delete([mntns])

    def AttachContainer(self, container):
        self.containers[container] = None

    def DetachContainer(self, container):
        """tracer.go:163-171: the Peek result, or the error's text as a one-element list."""
        try:
            self.containers[container] = self.Peek(container.Mntns)
        except LookupError as e:
            self.containers[container] = [str(e)]

    def collectResult(self) -> str:
        """tracer.go:173-179: json.MarshalIndent(map[name][]string, "", "  "); a container that was
        never detached marshals as null.  Containers that share a name keep one entry, as in
        the reference, here the last attached."""
        return go_marshal({c.Name: r for c, r in self.containers.items()}, indent="  ")

    def destroy(self):
        self.map.destroy()


# ------------------------------------------------------------------------------------
# traceloop (pkg/gadgets/traceloop/tracer/tracer.go, syscall_helpers.go, types/types.go)
# ------------------------------------------------------------------------------------
USE_NULL_BYTE_LENGTH = 0x0FFFFFFFFFFFFFFF      # traceloop.h:18
TRACELOOP_SYS_SAMPLE, TRACELOOP_CONT_SAMPLE = 100, 156   # alignSize(96), alignSize(152): tracer.go:86-92
# struct syscall_event_t / syscall_event_cont_t (traceloop.h:34-55): (name, offset, bytes)
TRACELOOP_SYS_FIELDS = [("args", 0, 48), ("mono_ts", 48, 8), ("boot_ts", 56, 8), ("pid", 64, 4), ("cpu", 68, 2),
                        ("id", 70, 2), ("comm", 72, 16), ("cont_nr", 88, 1), ("typ", 89, 1)]
TRACELOOP_CONT_FIELDS = [("param", 0, 128), ("mono_ts", 128, 8), ("length", 136, 8), ("index", 144, 1),
                         ("failed", 145, 1)]
TRACELOOP_SYS_BYTES, TRACELOOP_CONT_BYTES = 96, 152


def _traceloop_dtypes():
    import numpy as np
    sys_dt = np.dtype({"names": ["args", "mono_ts", "boot_ts", "pid", "cpu", "id", "comm", "cont_nr", "typ"],
                       "formats": [("<u8", 6), "<u8", "<u8", "<u4", "<u2", "<u2", ("u1", 16), "u1", "u1"],
                       "offsets": [o for _, o, _ in TRACELOOP_SYS_FIELDS], "itemsize": TRACELOOP_SYS_BYTES})
    cont_dt = np.dtype({"names": ["param", "mono_ts", "length", "index", "failed"],
                        "formats": [("u1", 128), "<u8", "<u8", "u1", "u1"],
                        "offsets": [o for _, o, _ in TRACELOOP_CONT_FIELDS], "itemsize": TRACELOOP_CONT_BYTES})
    return sys_dt, cont_dt


def traceloop_decode(samples):
    """The size switch of Read's callback (tracer.go:272-348) over raw samples (bytes-likes) in
    the order readOverWritable delivers them: a sample of 100 bytes is a syscall_event_t, one of
    156 a syscall_event_cont_t, any other size is dropped.  Returns two numpy structured arrays
    (fields as TRACELOOP_SYS_FIELDS / TRACELOOP_CONT_FIELDS), each in sample order."""
    import numpy as np
    sys_dt, cont_dt = _traceloop_dtypes()
    s, c = bytearray(), bytearray()
    for raw in samples:
        raw = bytes(raw)
        if len(raw) == TRACELOOP_SYS_SAMPLE:
            s += raw[:TRACELOOP_SYS_BYTES]
        elif len(raw) == TRACELOOP_CONT_SAMPLE:
            c += raw[:TRACELOOP_CONT_BYTES]
    return np.frombuffer(bytes(s), dtype=sys_dt), np.frombuffer(bytes(c), dtype=cont_dt)


_GO_ESC = {7: "\\a", 8: "\\b", 12: "\\f", 10: "\\n", 13: "\\r", 9: "\\t", 11: "\\v", 0x5C: "\\\\", 0x22: '\\"'}


def go_quote(b) -> str:
    """strconv.Quote of a Go string holding the bytes b (str: its UTF-8).  \\a \\b \\f \\n \\r \\t \\v
    \\\\ \\" are escaped; other bytes below 0x20, 0x7f and every byte of invalid UTF-8 print as \\xNN;
    printable runes (strconv.IsPrint: categories L, M, N, P, S and U+0020) are kept; other runes
    print as \\uNNNN below 0x10000 and \\UNNNNNNNN above.  Categories come from unicodedata, so
    the Unicode version is this interpreter's, not that of the Go release the reference was
    built with."""
    import unicodedata
    b = b.encode("utf-8") if isinstance(b, str) else bytes(b)
    out, i, n = ['"'], 0, len(b)
    while i < n:
        c0 = b[i]
        r, w = None, 1
        if c0 < 0x80:
            r = c0
        else:     # utf8.DecodeRuneInString: shortest form, no surrogates, at most U+10FFFF
            need = 2 if 0xC2 <= c0 <= 0xDF else 3 if 0xE0 <= c0 <= 0xEF else 4 if 0xF0 <= c0 <= 0xF4 else 0
            if need and i + need <= n:
                try:
                    r, w = ord(b[i:i + need].decode("utf-8")), need
                except UnicodeDecodeError:
                    r = None
        if r is None:
            out.append("\\x%02x" % c0)
        elif r in _GO_ESC:
            out.append(_GO_ESC[r])
        elif r == 0x20 or unicodedata.category(chr(r))[0] in "LMNPS":
            out.append(chr(r))
        elif r < 0x20 or r == 0x7F:
            out.append("\\x%02x" % r)
        elif r < 0x10000:
            out.append("\\u%04x" % r)
        else:
            out.append("\\U%08x" % r)
        i += w
    out.append('"')
    return "".join(out)


def _c_bytes(b, limit=None):
    """gadgets.FromCString / FromCStringN (helpers.go:76-97) on bytes, as bytes."""
    b = bytes(b)
    if limit is not None:
        if limit < 0:
            raise ValueError("traceloop: cont length converts to a negative int (the reference panics)")
        b = b[:limit]
    i = b.find(b"\0")
    return b if i < 0 else b[:i]


def traceloop_cont_param(param, length: int, failed: int) -> str:
    """A cont record's parameter text (tracer.go:326-336)."""
    if failed:
        s = b"(Failed to dereference pointer)"
    elif length == USE_NULL_BYTE_LENGTH:
        s = _c_bytes(param)
    else:
        s = _c_bytes(param, length - (1 << 64) if length >= 1 << 63 else length)
    return go_quote(s)


@dataclass
class SyscallDeclaration:
    """syscall_helpers.go:37-40: params are (position, name)."""
    name: str
    params: list = field(default_factory=list)

    def getParameterCount(self) -> int:
        return len(self.params) & 0xFF

    def getParameterName(self, i: int) -> str:
        if i >= len(self.params):
            raise IndexError(f"param number {i} out of bounds for syscall {self.name!r}")
        return self.params[i][1]


_TRACEFS_FIELD = None


def parseSyscall(name: str, format_text: str) -> SyscallDeclaration:
    """syscall_helpers.go:81-167 on the text of a tracefs `format` file: lines up to the first empty
    one are skipped; after it every line matching `\\s+field:TYPE NAME;` is a parameter, at position
    line index - 8, except __syscall_nr."""
    global _TRACEFS_FIELD
    if _TRACEFS_FIELD is None:
        import re
        _TRACEFS_FIELD = re.compile(r"[\t\n\f\r ]+field:(.*?) ([a-z_0-9]+);.*")
    params, skipped = [], False
    for idx, line in enumerate(format_text.split("\n")):
        if not skipped:
            if len(line) != 0:
                continue
            skipped = True
        m = _TRACEFS_FIELD.search(line)
        if m is None or m.group(2) == "__syscall_nr":
            continue
        params.append((idx - 8, m.group(2)))
    return SyscallDeclaration(name, params)


def relateSyscallName(name: str) -> str:
    """syscall_helpers.go:120-139: sys_enter_NAME -> the name in asm/unistd_64.h."""
    return {"newfstat": "fstat", "newlstat": "lstat", "newstat": "stat", "newuname": "uname",
            "sendfile64": "sendfile", "sysctl": "_sysctl", "umount": "umount2"}.get(name, name)


@dataclass
class SyscallParam:
    """types.go:26-29."""
    Name: str = ""
    Value: str = ""


@dataclass
class TraceloopEvent:
    """pkg/gadgets/traceloop/types/types.go:31-41 (eventtypes.Event + WithMountNsID flattened)."""
    Node: str = ""
    Namespace: str = ""
    Pod: str = ""
    Container: str = ""
    Timestamp: int = 0
    MountNsID: int = 0
    CPU: int = 0
    Pid: int = 0
    Comm: str = ""
    Syscall: str = ""
    Parameters: list = field(default_factory=list)
    Retval: int = 0


_TRACELOOP_NO_EXIT = ("exit", "exit_group", "rt_sigreturn")


def TraceloopColumns():
    """types.GetColumns() (types.go:51-91): the params and ret extractors; node, namespace, pod
    and container hidden.  Filtering or sorting by an extractor column is not supported, as for
    every extractor column."""
    from . import textcolumns as T
    cm = T.ColumnMap([(a, k, t) for a, k, t, _ in _COMMON_COLS[:4]] +
                     [("Timestamp", "int64", "timestamp,template:timestamp"), ("MountNsID", "uint64", "mntns,template:ns"),
                      ("CPU", "uint16", "cpu,width:3,fixed"), ("Pid", "uint32", "pid,template:pid"),
                      ("Comm", "string", "comm,template:comm"), ("Syscall", "string", "syscall,template:syscall"),
                      ("Parameters", "string", "params,width:40"), ("Retval", "int", "ret,width:3,fixed")])
    for a, _, t, tags in _COMMON_COLS[:4]:
        cm.cols[t.split(",")[0]].Tags = list(tags)
    cm.SetExtractor("params", lambda ev: ", ".join(f"{p.Name}={p.Value}" for p in ev.Parameters))
    cm.SetExtractor("ret", lambda ev: "X" if ev.Syscall in _TRACELOOP_NO_EXIT else str(int(ev.Retval)))
    for name in ("node", "namespace", "pod", "container"):
        cm.cols[name].Visible = False
    return cm


def traceloop_render(events, terminal_width: int = 0, columns=None) -> str:
    """The columns output of one Read."""
    from . import textcolumns as T
    return T.TransformIntoTable(T.TextColumnsFormatter(TraceloopColumns(), DefaultColumns=columns), events, terminal_width)


def traceloop_events(sys, cont, row, exit_row, cls, cont_rows, names, declarations, mntns=None, have_boot_ns=True,
                     boot_to_wall_ns=0):
    """The types.Event list of tracer.go:369-530 from the join's columns (host sequences: row,
    exit_row, cls per event, cont_rows six per event; 0xFFFFFFFF or -1: none) over the decoded
    records sys / cont (traceloop_decode).  mntns: per syscall row, or one number."""
    none = (0xFFFFFFFF, -1)
    out = []
    for j in range(len(row)):
        r = sys[int(row[j])]
        name = names.get(int(r["id"]))
        if name is None:
            if int(cls[j]) == 2:
                continue                                      # :502-507: best effort
            raise LookupError(f"getting name of syscall number {int(r['id'])}")
        ts = int(r["boot_ts"]) if have_boot_ns else int(r["mono_ts"])
        mn = mntns if mntns is None or isinstance(mntns, int) else int(mntns[int(row[j])])
        ev = TraceloopEvent(Timestamp=(ts + boot_to_wall_ns) if have_boot_ns else 0, MountNsID=mn or 0,
                            CPU=int(r["cpu"]), Pid=int(r["pid"]), Comm=_c_bytes(r["comm"].tobytes()).decode("utf-8", "replace"),
                            Syscall=name)
        if int(cls[j]) == 0:
            decl = declarations[name]
            decl = decl if isinstance(decl, SyscallDeclaration) else SyscallDeclaration(name, list(enumerate(decl)))
            for i in range(decl.getParameterCount()):
                value = "%d" % int(r["args"][i])              # i >= 6: the reference's slice has six
                cj = int(cont_rows[6 * j + i]) if i < 6 else -1
                if cj not in none:
                    c = cont[cj]
                    value = traceloop_cont_param(c["param"].tobytes(), int(c["length"]), int(c["failed"]))
                ev.Parameters.append(SyscallParam(decl.getParameterName(i), value))
            if int(exit_row[j]) not in none:
                ev.Retval = int(sys[int(exit_row[j])]["args"][0].astype("int64"))
        elif int(cls[j]) == 2:
            ev.Retval = int(r["args"][0].astype("int64"))
        out.append(ev)
    return out


class TraceloopTracer:
    """traceloop: the syscall flight recorder.  Attach / Detach / Delete as tracer.go:196-230 and
    :547-567; feed() stands for the BPF side writing raw samples into a container's ring in the
    order readOverWritable would deliver them (reading the ring is the caller's); Read(containerID)
    is Tracer.Read for one container, and ReadAll() runs one device join over the rows of every
    attached container and splits the events per container afterwards.

    names: {number: name} (default _syscalls.X86_64); declarations: {name: SyscallDeclaration or
    a list of parameter names} (parseSyscall / relateSyscallName build them from tracefs format
    files).  have_boot_ns=False is a kernel without bpf_ktime_get_boot_ns: events sort by the
    monotonic timestamp and carry Timestamp 0 (tracer.go:232-244, :538-542).  boot_to_wall_ns is
    WallTimeFromBootTime's offset, applied to every timestamp, zero included.  A Read consumes
    the samples it saw."""

    def __init__(self, declarations, names=None, have_boot_ns=True, boot_to_wall_ns=0, device="cuda"):
        from ._syscalls import X86_64
        self.names = dict(X86_64 if names is None else names)
        self.declarations = dict(declarations)
        by_name = {v: k for k, v in self.names.items()}
        self.nr = tuple(by_name.get(n, 0xFFFF) for n in _TRACELOOP_NO_EXIT)
        self.have_boot_ns, self.boot_to_wall_ns, self.device = have_boot_ns, boot_to_wall_ns, device
        self.readers: Dict[str, dict] = {}     # containerID -> {"mntns", "samples", "attached"}

    def Attach(self, containerID: str, mntns: int):
        self.readers[containerID] = {"mntns": int(mntns), "samples": [], "attached": True}

    def Detach(self, mntns: int):
        """The perf buffer leaves the BPF map: nothing more is recorded for the namespace."""
        hit = [r for r in self.readers.values() if r["mntns"] == int(mntns) and r["attached"]]
        if not hit:
            raise LookupError(f"error removing perf buffer from map with mntnsID {mntns}")
        for r in hit:
            r["attached"] = False

    def Delete(self, containerID: str):
        if self.readers.pop(containerID, None) is None:
            raise LookupError(f"no reader for containerID {containerID}")

    def feed(self, containerID: str, samples):
        r = self.readers.get(containerID)
        if r is None:
            raise LookupError(f'no perf reader for "{containerID}"')
        if r["attached"]:
            r["samples"] += [bytes(s) for s in samples]

    def _device_cols(self, sys, cont):
        import numpy as np
        torch = torch_mod()
        out = []
        for arr, nbytes, fields in ((sys, TRACELOOP_SYS_BYTES, [("mono_ts", 48, 8, torch.uint64), ("boot_ts", 56, 8, torch.uint64),
                                                                ("pid", 64, 4, torch.int32), ("id", 70, 2, torch.int16),
                                                                ("typ", 89, 1, torch.uint8)]),
                                    (cont, TRACELOOP_CONT_BYTES, [("mono_ts", 128, 8, torch.uint64), ("index", 144, 1, torch.uint8)])):
            n = len(arr)
            if n == 0:
                out.append({f[0]: torch.empty(0, dtype=f[3], device=self.device) for f in fields})
                continue
            raw = torch.from_numpy(np.frombuffer(arr.tobytes(), dtype=np.uint8).copy()).to(self.device)
            out.append(engine.ingest_aos(raw, n, nbytes, fields))
        return out

    def _check_enters(self, sys):
        """tracer.go:364-384: an enter without a name or a declaration fails the whole Read."""
        for i in sorted({int(x) for x in sys["id"][sys["typ"] == 0]}):
            name = self.names.get(i)
            if name is None:
                raise LookupError(f"getting name of syscall number {i}")
            if name not in self.declarations:
                raise LookupError("getting syscall definition")

    def _join(self, sys, cont, mntns_s=None, mntns_c=None):
        torch = torch_mod()
        self._check_enters(sys)
        if len(sys) == 0:
            return []
        ds, dc = self._device_cols(sys, cont)
        dev_mn = lambda a: None if a is None else torch.from_numpy(a.view("int64")).to(self.device)   # noqa: E731
        j = engine.traceloop_join(ds["mono_ts"], ds["boot_ts"] if self.have_boot_ns else ds["mono_ts"], ds["typ"],
                                  ds["id"], ds["pid"], mntns=dev_mn(mntns_s), c_mono_ts=dc["mono_ts"],
                                  c_index=dc["index"], c_mntns=dev_mn(mntns_c), nr=self.nr)
        return j

    def Read(self, containerID: str) -> List[TraceloopEvent]:
        r = self.readers.get(containerID)
        if r is None:
            raise LookupError(f'no perf reader for "{containerID}"')
        sys, cont = traceloop_decode(r["samples"])
        j = self._join(sys, cont)
        r["samples"] = []
        if not len(sys):
            return []
        return traceloop_events(sys, cont, host(j["row"]), host(j["exit"]), host(j["cls"]), host(j["cont"]).reshape(-1),
                                self.names, self.declarations, r["mntns"], self.have_boot_ns, self.boot_to_wall_ns)

    def ReadAll(self) -> Dict[str, List[TraceloopEvent]]:
        """One join over every container's rows; {containerID: events}.  An enter without a name
        or a declaration in any container fails the call."""
        import numpy as np
        ids = list(self.readers)
        dec = [traceloop_decode(self.readers[c]["samples"]) for c in ids]
        # one decode of every container's samples (np.concatenate would repack the padded records)
        sys, cont = traceloop_decode([s for c in ids for s in self.readers[c]["samples"]])
        mn = lambda k: np.concatenate([np.full(len(d[k]), self.readers[c]["mntns"], np.uint64)   # noqa: E731
                                       for c, d in zip(ids, dec)]) if dec else np.zeros(0, np.uint64)
        mntns_s, mntns_c = mn(0), mn(1)
        owner = np.concatenate([np.full(len(d[0]), i, np.int64) for i, d in enumerate(dec)]) if dec else np.zeros(0, np.int64)
        j = self._join(sys, cont, mntns_s, mntns_c)
        for c in ids:
            self.readers[c]["samples"] = []
        out = {c: [] for c in ids}
        if not len(sys):
            return out
        row, ex, cls, cr = host(j["row"]), host(j["exit"]), host(j["cls"]), host(j["cont"]).reshape(-1, 6)
        for i, c in enumerate(ids):
            sel = np.nonzero(owner[row] == i)[0]
            out[c] = traceloop_events(sys, cont, row[sel], ex[sel], cls[sel], cr[sel].reshape(-1), self.names,
                                      self.declarations, self.readers[c]["mntns"], self.have_boot_ns, self.boot_to_wall_ns)
        return out


# ------------------------------------------------------------------------------------
# trace capabilities (pkg/gadgets/trace/capabilities)
# ------------------------------------------------------------------------------------
CAP_ENTER, CAP_EXIT, SYS_ENTER, SYS_EXIT = 0, 1, 2, 3      # the four probes of capable.bpf.c, as batch kinds

# The kernel's capability names (include/uapi/linux/capability.h, CAP_CHOWN = 0 ..
# CAP_CHECKPOINT_RESTORE = 40) without their prefix: CapName is the upper-case form
# (tracer.go:59-101) and CapsNames the lower-case one.
CAPABILITY_NAMES = (
    "CHOWN", "DAC_OVERRIDE", "DAC_READ_SEARCH", "FOWNER", "FSETID", "KILL", "SETGID", "SETUID", "SETPCAP",
    "LINUX_IMMUTABLE", "NET_BIND_SERVICE", "NET_BROADCAST", "NET_ADMIN", "NET_RAW", "IPC_LOCK", "IPC_OWNER",
    "SYS_MODULE", "SYS_RAWIO", "SYS_CHROOT", "SYS_PTRACE", "SYS_PACCT", "SYS_ADMIN", "SYS_BOOT", "SYS_NICE",
    "SYS_RESOURCE", "SYS_TIME", "SYS_TTY_CONFIG", "MKNOD", "LEASE", "AUDIT_WRITE", "AUDIT_CONTROL", "SETFCAP",
    "MAC_OVERRIDE", "MAC_ADMIN", "SYSLOG", "WAKE_ALARM", "BLOCK_SUSPEND", "AUDIT_READ", "PERFMON", "BPF",
    "CHECKPOINT_RESTORE")
CAP_LAST_CAP = len(CAPABILITY_NAMES) - 1

CAPABILITIES_SKIP_NR = {"amd64": (60, 231, 15), "arm64": (93, 94, 139)}   # exit, exit_group, rt_sigreturn (:202-212)
CAPABILITIES_COLS = ("kind", "pid_tgid", "mntns", "ts", "nr", "cap", "cap_opt", "cred_is_real", "current_userns",
                     "target_userns", "cap_effective", "ret", "uid", "comm")


def kernelVersion(a: int, b: int, c: int) -> int:
    """tracer.go:224-230 (the KERNEL_VERSION macro)."""
    return (a << 16) + (b << 8) + min(c, 255)


def capabilityName(cap: int) -> str:
    """tracer.go:259-265."""
    return CAPABILITY_NAMES[cap] if 0 <= cap <= CAP_LAST_CAP else f"UNKNOWN ({cap})"


def capsNames(capsBitField: int) -> List[str]:
    """tracer.go:232-241: the lower-case names of the bits set, up to CAP_LAST_CAP."""
    return [CAPABILITY_NAMES[i].lower() for i in range(CAP_LAST_CAP + 1) if (1 << i) & capsBitField]


@dataclass
class CapabilitiesEvent:
    """pkg/gadgets/trace/capabilities/types/types.go:35-52 (eventtypes.Event + WithMountNsID
    flattened).  InsetID is None on kernels before 5.1.0."""
    Node: str = ""
    Namespace: str = ""
    Pod: str = ""
    Container: str = ""
    Timestamp: int = 0
    MountNsID: int = 0
    Pid: int = 0
    Comm: str = ""
    Syscall: str = ""
    UID: int = 0
    Cap: int = 0
    CapName: str = ""
    Audit: int = 0
    Verdict: str = ""
    InsetID: Optional[bool] = None
    TargetUserNs: int = 0
    CurrentUserNs: int = 0
    Caps: int = 0
    CapsNames: list = field(default_factory=list)


def capabilities_event(kernel_version: int, names, pid, uid, mntns, comm, ret, ts, current_userns, target_userns,
                       cap_effective, cap, cap_opt, syscall, boot_to_wall_ns=0) -> CapabilitiesEvent:
    """tracer.go:257-318 for one cap_event; syscall -1 (no current_syscall entry, or a number
    without a name) renders ""."""
    if kernel_version >= kernelVersion(5, 1, 0):
        audit = 1 if (cap_opt & 0b10) == 0 else 0
        inset = (cap_opt & 0b100) != 0
    else:
        audit, inset = cap_opt, None
    nr = int(syscall) & 0xFFFFFFFF                    # libseccomp.ScmpSyscall is an int32
    nr = nr - (1 << 32) if nr >= 1 << 31 else nr
    return CapabilitiesEvent(Timestamp=int(ts) + boot_to_wall_ns, MountNsID=int(mntns), Pid=int(pid),
                             Comm=FromCString(comm), Syscall=names.get(nr, "") if nr >= 0 else "", UID=int(uid),
                             Cap=int(cap), CapName=capabilityName(int(cap)), Audit=int(audit),
                             Verdict="Allow" if int(ret) == 0 else "Deny", InsetID=inset,
                             TargetUserNs=int(target_userns), CurrentUserNs=int(current_userns),
                             Caps=int(cap_effective), CapsNames=capsNames(int(cap_effective)))


def CapabilitiesColumns():
    """types.GetColumns() (types.go:54-73): the insetid, caps and capsnames extractors."""
    from . import textcolumns as T
    cm = T.ColumnMap([(a, k, t) for a, k, t, _ in _COMMON_COLS[:4]] +
                     [("Timestamp", "int64", "timestamp,template:timestamp"), ("MountNsID", "uint64", "mntns,template:ns"),
                      ("Pid", "uint32", "pid,template:pid"), ("Comm", "string", "comm,template:comm"),
                      ("Syscall", "string", "syscall,template:syscall"), ("UID", "uint32", "uid,minWidth:6"),
                      ("Cap", "int", "cap,width:3,fixed"), ("CapName", "string", "capName,width:18,fixed"),
                      ("Audit", "int", "audit,minWidth:5"), ("Verdict", "string", "verdict,width:7,fixed"),
                      ("InsetID", "bool", "insetid,width:7,fixed,hide"),
                      ("TargetUserNs", "uint64", "targetuserns,template:ns"),
                      ("CurrentUserNs", "uint64", "currentuserns,template:ns"), ("Caps", "uint64", "caps,hide"),
                      ("CapsNames", "string", "capsnames,hide")])
    for a, _, t, tags in _COMMON_COLS[:4]:
        cm.cols[t.split(",")[0]].Tags = list(tags)
    cm.SetExtractor("insetid", lambda ev: "N/A" if ev.InsetID is None else ("true" if ev.InsetID else "false"))
    cm.SetExtractor("caps", lambda ev: "%x" % ev.Caps)
    cm.SetExtractor("capsnames", lambda ev: ",".join(ev.CapsNames))
    for name in ("node", "namespace", "pod", "container"):
        cm.cols[name].Visible = False
    return cm


def capabilities_render(events, terminal_width: int = 0, columns=None) -> str:
    """The columns output of a list of events."""
    from . import textcolumns as T
    return T.TransformIntoTable(T.TextColumnsFormatter(CapabilitiesColumns(), DefaultColumns=columns), events,
                                terminal_width)


class TraceCapabilitiesTracer:
    """trace capabilities from its four probes' own rows (capable.bpf.c:87-248), joined on the
    device by igx_lw_join: the cap_capable kprobe is SET_A on the thread's `start` entry, its
    kretprobe TAKE_A, sys_enter SET_B on `current_syscall` and sys_exit CLEAR_B.

    feed(batch) takes device columns (CAPABILITIES_COLS) of probe rows in stream order: kind
    (uint8: CAP_ENTER, CAP_EXIT, SYS_ENTER, SYS_EXIT), pid_tgid, mntns, ts (boot ns), nr,
    current_userns, target_userns, cap_effective (u64), cap, cap_opt, ret (i32), uid (u32),
    cred_is_real (u8: cred == real_cred, :101-107), comm ((n, 16) u8).  It applies the probes' own
    filters, --unique through igx_intern_add_first on (cap, mntns), joins, gathers the events on
    the device and returns them in stream order.  Rows still held in a map after a batch are
    carried into the next one; more than pending_cap of them raises IgxError(IGX_ENOSPC).

    kernel_version: (a, b, c) or a version code.  names: {number: name} for Syscall (default
    _syscalls.X86_64); goarch selects the numbers sys_enter skips.  my_pid / targ_pid: -1 is
    "none", as the BPF constants.  mntns_filter: an iterable of mount namespace ids, or None.
    boot_to_wall_ns: WallTimeFromBootTime's offset."""

    def __init__(self, Unique=False, AuditOnly=True, kernel_version=(5, 15, 0), mntns_filter=None, my_pid=-1,
                 targ_pid=-1, goarch="amd64", seen_capacity=1 << 16, names=None, pending_cap=1 << 20,
                 boot_to_wall_ns=0, device="cuda"):
        from ._syscalls import X86_64
        self.Unique, self.AuditOnly = bool(Unique), bool(AuditOnly)
        self.kernel_version = kernel_version if isinstance(kernel_version, int) else kernelVersion(*kernel_version)
        self.mntns_filter = None if mntns_filter is None else sorted(int(x) for x in mntns_filter)
        self.my_pid, self.targ_pid = int(my_pid), int(targ_pid)
        if goarch not in CAPABILITIES_SKIP_NR:
            raise ValueError("The trace capabilities gadget is not supported on your architecture.")
        self.skip_nr = CAPABILITIES_SKIP_NR[goarch]
        self.names = dict(X86_64 if names is None else names)
        self.pending_cap, self.boot_to_wall_ns, self.device = int(pending_cap), int(boot_to_wall_ns), device
        self._seen = engine.Interner(16, int(seen_capacity)) if self.Unique else None
        self._carry = None            # {column: tensor} of the rows still in `start` / `current_syscall`

    def _valid(self, c):
        """The probes' filters, in their order, as one uint8 mask over the new rows."""
        torch = torch_mod()
        i64 = lambda t: t.view(torch.int64) if t.dtype == torch.uint64 else t.to(torch.int64)   # noqa: E731
        kind = c["kind"]
        cap_e, sys_e = kind == CAP_ENTER, kind == SYS_ENTER
        in_ns = None
        if self.mntns_filter is not None:              # :98-99, :229-230
            import numpy as np
            ids = torch.from_numpy(np.array(self.mntns_filter, np.uint64).view(np.int64)).to(kind.device)
            in_ns = torch.isin(i64(c["mntns"]), ids)
        pid = (i64(c["pid_tgid"]) >> 32) & 0xFFFFFFFF
        ok_cap = c["cred_is_real"] != 0                                         # :101-107
        ok_cap &= pid != (self.my_pid & 0xFFFFFFFF)                             # :112-113 (pid is a __u32)
        if self.targ_pid != -1:
            ok_cap &= pid == (self.targ_pid & 0xFFFFFFFF)                       # :115-116
        if self.AuditOnly:                                                      # :118-126
            opt = c["cap_opt"].to(torch.int64)
            ok_cap &= ((opt & 0b10) == 0) if self.kernel_version >= kernelVersion(5, 1, 0) else (opt != 0)
        nr = i64(c["nr"]) & 0xFFFFFFFF                                          # skip_exit_probe(int nr), :214-218
        ok_sys = (nr != self.skip_nr[0]) & (nr != self.skip_nr[1]) & (nr != self.skip_nr[2])
        if in_ns is not None:
            ok_cap &= in_ns
            ok_sys &= in_ns
        return (torch.where(cap_e, ok_cap, torch.where(sys_e, ok_sys, kind <= SYS_EXIT))).to(torch.uint8)

    def _unique(self, c, valid):
        """:128-139: of the CAP_ENTER rows that passed the filters, only the first of each
        (cap, mntns) stays; the others return before `start` is written."""
        torch = torch_mod()
        cap_e = (c["kind"] == CAP_ENTER) & (valid != 0)
        rows = torch.stack([c["cap"].to(torch.int64) & 0xFFFFFFFF,
                            c["mntns"].view(torch.int64) if c["mntns"].dtype == torch.uint64 else c["mntns"].to(torch.int64)],
                           dim=1).contiguous().view(torch.uint8)
        _, first = self._seen.add(rows, cap_e.to(torch.uint8), first=True)
        return torch.where(c["kind"] == CAP_ENTER, first, valid)

    def feed(self, batch: dict, n: Optional[int] = None) -> List[CapabilitiesEvent]:
        torch = torch_mod()
        n = int(batch["kind"].shape[0]) if n is None else n
        c = {k: batch[k][:n] for k in CAPABILITIES_COLS}
        valid = self._valid(c)
        if self.Unique and n:
            valid = self._unique(c, valid)
        if self._carry is not None:
            # the carried rows were admitted when they came: they pass no filter and no unique gate again
            valid = torch.cat([torch.ones(self._carry["kind"].shape[0], dtype=torch.uint8, device=valid.device), valid])
            c = {k: _cat_rows(self._carry[k], v) for k, v in c.items()}
        if c["kind"].shape[0] == 0:
            return []
        lut = torch.tensor([_abi.LW_SET_A, _abi.LW_TAKE_A, _abi.LW_SET_B, _abi.LW_CLEAR_B] + [255] * 252,
                           dtype=torch.uint8, device=c["kind"].device)
        j = engine.lw_join(c["pid_tgid"], lut[c["kind"].to(torch.int64)], valid, pend_cap=self.pending_cap)
        if j["n_pend"] > self.pending_cap:
            raise _abi.IgxError(_abi.IGX_ENOSPC, f"trace capabilities: {j['n_pend']} map entries exceed "
                                                 f"pending_cap={self.pending_cap}")
        names = list(c)
        carry = dict(zip(names, engine.take([c[k] for k in names], j["pend"])))
        self._carry = carry if j["n_pend"] else None
        if j["n_take"] == 0:
            return []
        pid_tgid, uid, mntns, comm, ret, ts = engine.take([c[k] for k in ("pid_tgid", "uid", "mntns", "comm", "ret", "ts")],
                                                          j["take"])
        cur, tgt, eff, cap, opt = engine.take([c[k] for k in ("current_userns", "target_userns", "cap_effective", "cap",
                                                              "cap_opt")], j["a"])
        nr, = engine.take([c["nr"]], j["b"], pad=True)
        # :184-189: without a current_syscall entry the syscall is -1; the gathered zero row would read as syscall 0
        nr = torch.where(j["b"] == -1, torch.full_like(nr.view(torch.int64), -1), nr.view(torch.int64))
        h = [host(t) for t in (pid_tgid, uid, mntns, comm, ret, ts, cur, tgt, eff, cap, opt, nr)]
        return [capabilities_event(self.kernel_version, self.names, int(h[0][i]) >> 32, h[1][i], h[2][i],
                                   h[3][i].tobytes(), h[4][i], h[5][i], h[6][i], h[7][i], h[8][i], h[9][i], h[10][i],
                                   h[11][i], self.boot_to_wall_ns) for i in range(len(h[0]))]

    @property
    def pending(self):
        """Map entries alive (rows carried into the next batch)."""
        return 0 if self._carry is None else int(self._carry["kind"].shape[0])

    def destroy(self):
        if self._seen is not None:
            self._seen.destroy()
            self._seen = None
        self._carry = None


# ------------------------------------------------------------------------------------
# trace tcp: pkg/gadgets/trace/tcp (tracer/bpf/tcptracer.bpf.c, tracer/tracer.go:198-234,
# types/types.go:22-55)
# ------------------------------------------------------------------------------------
TCP_TRACE_COLS = engine.TCP_ROW_FIELDS + ("ts", "comm")
_TCP_OPERATIONS = {_abi.TCP_EV_ACCEPT: "accept", _abi.TCP_EV_CLOSE: "close", 3: "connect"}


def Htons(hs: int) -> int:
    """helpers.go:105-109 on a little-endian host: the two bytes of a uint16 swapped."""
    hs = int(hs) & 0xFFFF
    return ((hs & 0xFF) << 8) | (hs >> 8)


@dataclass
class TcpEvent:
    """pkg/gadgets/trace/tcp/types/types.go:22-34 (eventtypes.Event + WithMountNsID flattened)."""
    Node: str = ""
    Namespace: str = ""
    Pod: str = ""
    Container: str = ""
    Timestamp: int = 0
    Type: str = "normal"
    MountNsID: int = 0
    Operation: str = ""
    Pid: int = 0
    Comm: str = ""
    IPVersion: int = 0
    Saddr: str = ""
    Daddr: str = ""
    Sport: int = 0
    Dport: int = 0


_TCP_EVENT_JSON = _COMMON_JSON[:4] + [("Timestamp", "timestamp", True), ("Type", "type", False),
                                      ("MountNsID", "mountnsid", True), ("Operation", "operation", True),
                                      ("Pid", "pid", True), ("Comm", "comm", True), ("IPVersion", "ipversion", True),
                                      ("Saddr", "saddr", True), ("Daddr", "daddr", True), ("Sport", "sport", True),
                                      ("Dport", "dport", True)]


def tcp_event(op, family, tuple40, pid, mntns, comm, ts, boot_to_wall_ns=0) -> TcpEvent:
    """tracer.go:198-228 for one event of the probes: op is the event type (1 accept, 2 close,
    3 connect), tuple40 the tuple_key_t bytes the probe filled the event from (fill_event,
    tcptracer.bpf.c:124-144)."""
    t = bytes(tuple40)
    v = 4 if int(family) == AF_INET else 6 if int(family) == AF_INET6 else 0
    return TcpEvent(Timestamp=int(ts) + boot_to_wall_ns, MountNsID=int(mntns), Operation=_TCP_OPERATIONS.get(int(op), ""),
                    Pid=int(pid), Comm=FromCString(comm), IPVersion=v, Saddr=IPStringFromBytes(t[0:16], v),
                    Daddr=IPStringFromBytes(t[16:32], v), Sport=Htons(int.from_bytes(t[32:34], "little")),
                    Dport=Htons(int.from_bytes(t[34:36], "little")))


def tcp_event_json(ev: TcpEvent) -> str:
    """json.Marshal of one event (the struct tags of types.go:22-34 and pkg/types/types.go)."""
    from . import textcolumns as T
    return T.marshal(ev, _TCP_EVENT_JSON)


def TraceTcpColumns():
    """types.GetColumns() (types.go:36-55): the `t` extractor maps the operation to A / C / X / U."""
    from . import textcolumns as T
    cm = T.ColumnMap([(a, k, t) for a, k, t, _ in _COMMON_COLS[:4]] +
                     [("Timestamp", "int64", "timestamp,template:timestamp"), ("MountNsID", "uint64", "mntns,template:ns"),
                      ("Operation", "string", "t,width:1,fixed"), ("Pid", "uint32", "pid,template:pid"),
                      ("Comm", "string", "comm,template:comm"), ("IPVersion", "int", "ip,width:2,fixed"),
                      ("Saddr", "string", "saddr,template:ipaddr"), ("Daddr", "string", "daddr,template:ipaddr"),
                      ("Sport", "uint16", "sport,template:ipport"), ("Dport", "uint16", "dport,template:ipport")])
    for a, _, t, tags in _COMMON_COLS[:4]:
        cm.cols[t.split(",")[0]].Tags = list(tags)
    cm.SetExtractor("t", lambda ev: {"accept": "A", "connect": "C", "close": "X", "unknown": "U"}.get(ev.Operation, "U"))
    for name in ("node", "namespace", "pod", "container"):
        cm.cols[name].Visible = False
    return cm


def tcp_render(events, terminal_width: int = 0, columns=None) -> str:
    """The columns output of a list of events."""
    from . import textcolumns as T
    return T.TransformIntoTable(T.TextColumnsFormatter(TraceTcpColumns(), DefaultColumns=columns), events,
                                terminal_width)


class TraceTcpTracer:
    """trace tcp from its probes' own rows (tcptracer.bpf.c), on the device: igx_tcp_classify
    applies fill_tuple and filter_event per row, the connect events run through igx_chain_join
    (`sockets` keyed by the thread, then `tuplepid` keyed by the tuple), accept and close events
    are per-row filters.

    feed(batch) takes device columns (TCP_TRACE_COLS) of probe rows in stream order: probe (uint8,
    _abi.TCP_*), tid, pid, uid (u32), mntns (u64), ret (i32), state (u8), family (u16), netns (u32),
    saddr, daddr ((n, 16) u8), dport, sport, num (u16, as the socket holds them), ts (u64, boot ns),
    comm ((n, 16) u8).  It returns the events in the order of the rows that emit them (perf-ring
    order).  A connect event has the tuple, family and timestamp of the tcp_set_state row and the
    pid / mntns / comm of the connect-return row (:319-321).  Rows still in a map after a batch are
    carried into the next one -- an admitted connect-return as IGX_CJ_HELD -- and meet no filter
    again; more than pending_cap of them raises IgxError(IGX_ENOSPC).

    The tuples become igx_chain_join's key2 through a fresh engine.Interner(40) per batch: carried
    rows are fed again in front, so ids need not outlive a batch.  mntns_filter: an iterable of up
    to 1024 mount namespace ids, or None.  filter_pid 0 and filter_uid -1 are "none", as the BPF
    constants.  boot_to_wall_ns: WallTimeFromBootTime's offset."""

    _CARRIED = TCP_TRACE_COLS + ("_kind", "_tuple", "_key1")

    def __init__(self, mntns_filter=None, filter_pid=0, filter_uid=-1, pending_cap=1 << 20, boot_to_wall_ns=0):
        self.mntns_filter = None if mntns_filter is None else sorted(set(int(x) for x in mntns_filter))
        if self.mntns_filter is not None and len(self.mntns_filter) > 1024:
            raise ValueError("trace tcp: the mount namespace filter holds at most 1024 ids")
        self.filter_pid, self.filter_uid = int(filter_pid), int(filter_uid)
        self.pending_cap, self.boot_to_wall_ns = int(pending_cap), int(boot_to_wall_ns)
        self._carry = None            # {column: tensor} of the rows still in `sockets` / `tuplepid`
        self._ns = None

    def _classify(self, c):
        torch = torch_mod()
        dev = c["probe"].device
        if self.mntns_filter is not None and len(self.mntns_filter) == 0:
            # an empty tensor has no address to pass, and igx_tcp_classify reads a null set as "no filter"
            raise ValueError("trace tcp: an empty mount namespace filter passes nothing; pass None for no filter")
        if self.mntns_filter is not None and (self._ns is None or self._ns.device != dev):
            import numpy as np
            self._ns = torch.from_numpy(np.array(self.mntns_filter, np.uint64).view(np.int64)).to(dev)
        return engine.tcp_classify(c, self.filter_pid, self.filter_uid, self._ns)

    def feed(self, batch: dict, n: Optional[int] = None) -> List[TcpEvent]:
        torch = torch_mod()
        n = int(batch["probe"].shape[0]) if n is None else n
        c = {k: batch[k][:n] for k in TCP_TRACE_COLS}
        cl = self._classify(c)
        c["_kind"], c["_tuple"], c["_key1"], event = cl["kind"], cl["tuple"], cl["key1"], cl["event"]
        if self._carry is not None:
            # the carried rows were admitted when they came: no filter again, and their own events are out
            event = torch.cat([torch.zeros(self._carry["_kind"].shape[0], dtype=torch.uint8, device=event.device), event])
            c = {k: _cat_rows(self._carry[k], v) for k, v in c.items()}
        total = int(c["_kind"].shape[0])
        if total == 0:
            return []
        kind = c["_kind"]
        keyed = ((kind == _abi.CJ_PASS) | (kind == _abi.CJ_HELD) | (kind == _abi.CJ_TAKE) | (kind == _abi.CJ_DROP))
        interner = engine.Interner(_abi.TCP_TUPLE_BYTES, total)
        try:
            key2 = interner.add(c["_tuple"], keyed.to(torch.uint8)).to(torch.int64)
            j = engine.chain_join(c["_key1"], key2, kind, pend_cap=self.pending_cap)
        finally:
            interner.destroy()
        if j["n_pend"] > self.pending_cap:
            raise _abi.IgxError(_abi.IGX_ENOSPC, f"trace tcp: {j['n_pend']} map entries exceed "
                                                 f"pending_cap={self.pending_cap}")
        if j["n_pend"]:
            names = list(c)
            carry = dict(zip(names, engine.take([c[k] for k in names], j["pend"])))
            carry["_kind"] = torch.where(carry["_kind"] == _abi.CJ_PASS, torch.full_like(carry["_kind"], _abi.CJ_HELD),
                                         carry["_kind"])
            self._carry = carry
        else:
            self._carry = None
        # one op per emitting row, and the row its task fields come from; nonzero() keeps row order
        op = event.clone()
        src = torch.arange(total, dtype=torch.int32, device=op.device)
        if j["n_take"]:
            t64 = j["take"].to(torch.int64)
            op[t64] = 3
            src[t64] = j["pass"]
        rows = torch.nonzero(op).flatten().to(torch.int32)
        if rows.numel() == 0:
            return []
        ops, tup, fam, ts = engine.take([op, c["_tuple"], c["family"], c["ts"]], rows)
        pid, mntns, comm = engine.take([c["pid"], c["mntns"], c["comm"]], src[rows.to(torch.int64)])
        h = [host(t) for t in (ops, fam, tup, pid, mntns, comm, ts)]
        return [tcp_event(h[0][i], h[1][i], h[2][i].tobytes(), h[3][i], h[4][i], h[5][i].tobytes(), h[6][i],
                          self.boot_to_wall_ns) for i in range(len(h[0]))]

    @property
    def pending(self):
        """Map entries alive (rows carried into the next batch)."""
        return 0 if self._carry is None else int(self._carry["_kind"].shape[0])

    def destroy(self):
        self._carry = None
