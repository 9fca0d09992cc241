"""Sequential restatement of trace tcp (pkg/gadgets/trace/tcp/tracer/bpf/tcptracer.bpf.c), written
from the BPF source with its line cites: the probes' per-row rules (fill_tuple, filter_event), the
two maps `sockets` and `tuplepid` as two Python dicts, and igx_chain_join's contract
(include/igx.h) over already classified rows.  A helper for the tests, not a test module.

Rows are a dict of numpy columns: probe u8, tid / pid / uid u32, mntns u64, ret i32, state u8,
family u16, netns u32, saddr / daddr (n, 16) u8, dport / sport / num u16 (as the socket holds them),
and for the gadget ts u64 and comm (n, 16) u8."""
import numpy as np

ENTER, PASS, ABORT, TAKE, DROP, HELD, NO_KIND = 0, 1, 2, 3, 4, 5, 255
P_ENTER, P_RETURN, P_CLOSE, P_STATE, P_ACCEPT = 0, 1, 2, 3, 4
EV_NONE, EV_ACCEPT, EV_CLOSE = 0, 1, 2
AF_INET, AF_INET6 = 2, 10
ESTABLISHED, SYN_SENT, SYN_RECV, CLOSE, NEW_SYN_RECV = 1, 2, 3, 7, 12
FIELDS = ("probe", "tid", "pid", "uid", "mntns", "ret", "state", "family", "netns", "saddr", "daddr", "dport",
          "sport", "num")
DTYPES = dict(probe=np.uint8, tid=np.uint32, pid=np.uint32, uid=np.uint32, mntns=np.uint64, ret=np.int32,
              state=np.uint8, family=np.uint16, netns=np.uint32, saddr=np.uint8, daddr=np.uint8, dport=np.uint16,
              sport=np.uint16, num=np.uint16)
Z4, Z16 = bytes(4), bytes(16)


# ---- the probes' own rules ---------------------------------------------------------------------
def fill_tuple(rows, i, family):
    """:79-122.  Returns (complete, key): key is the 40 bytes of tuple_key_t as far as they were
    filled when fill_tuple returned."""
    sa = da = Z16
    sport = dport = 0
    netns = int(rows["netns"][i])                                   # :84

    def key():
        return sa + da + sport.to_bytes(2, "little") + dport.to_bytes(2, "little") + netns.to_bytes(4, "little")

    s, d = bytes(rows["saddr"][i]), bytes(rows["daddr"][i])
    if family == AF_INET:
        sa = s[:4] + bytes(12)                                      # :88
        if s[:4] == Z4:
            return False, key()                                     # :89-90
        da = d[:4] + bytes(12)                                      # :92
        if d[:4] == Z4:
            return False, key()
    elif family == AF_INET6:
        sa = s                                                      # :98
        if s == Z16:
            return False, key()
        da = d                                                      # :102
        if d == Z16:
            return False, key()
    else:
        return False, key()                                         # :109-110
    dport = int(rows["dport"][i])                                   # :113
    if dport == 0:
        return False, key()
    sport = int(rows["sport"][i])                                   # :117
    if sport == 0:
        return False, key()
    return True, key()


def filter_event(rows, i, filter_pid=0, filter_uid=-1, mntns=None):
    """:147-166: True when the event is to be skipped.  mntns: None or a collection of ids."""
    if int(rows["family"][i]) not in (AF_INET, AF_INET6):
        return True
    if mntns is not None and int(rows["mntns"][i]) not in mntns:
        return True
    if filter_pid and int(rows["pid"][i]) != filter_pid:
        return True
    if (filter_uid & 0xFFFFFFFF) != 0xFFFFFFFF and int(rows["uid"][i]) != (filter_uid & 0xFFFFFFFF):
        return True
    return False


def classify_row(rows, i, filter_pid=0, filter_uid=-1, mntns=None):
    """(kind, event, key): what row i is for the chain join, the event it emits on its own, and its
    tuple key (40 zero bytes unless the row is PASS / TAKE / DROP or has an event)."""
    p = int(rows["probe"][i])
    fam = int(rows["family"][i])
    none = (NO_KIND, EV_NONE, bytes(40))
    flt = (filter_pid, filter_uid, mntns)
    if p == P_ENTER:                                                # :168-187
        return none if filter_event(rows, i, *flt) else (ENTER, EV_NONE, bytes(40))
    if p == P_RETURN:                                               # :189-227; no filter_event
        if int(rows["ret"][i]) != 0:
            return (ABORT, EV_NONE, bytes(40))                      # :207-208
        ok, key = fill_tuple(rows, i, fam)
        return (PASS, EV_NONE, key) if ok else (ABORT, EV_NONE, bytes(40))
    if p == P_STATE:                                                # :296-330; no filter_event
        st = int(rows["state"][i])
        if st not in (ESTABLISHED, CLOSE):
            return none                                             # :303-304 (a delete of the zero key)
        ok, key = fill_tuple(rows, i, fam)
        if not ok:
            return none                                             # a key with a zero field is never stored
        return (DROP if st == CLOSE else TAKE, EV_NONE, key)
    if p == P_CLOSE:                                                # :253-294
        if filter_event(rows, i, *flt):
            return none
        if int(rows["state"][i]) in (SYN_SENT, SYN_RECV, NEW_SYN_RECV):
            return none
        ok, key = fill_tuple(rows, i, fam)
        return (NO_KIND, EV_CLOSE, key) if ok else none
    if p == P_ACCEPT:                                               # :332-372
        if filter_event(rows, i, *flt):
            return none
        _, key = fill_tuple(rows, i, fam)                           # :357: result ignored
        num = int(rows["num"][i])
        sport = ((num & 0xFF) << 8) | (num >> 8)                    # :358 bpf_ntohs
        key = key[:32] + sport.to_bytes(2, "little") + key[34:]
        if key[:16] == Z16 or key[16:32] == Z16 or key[34:36] == bytes(2) or sport == 0:
            return none                                             # :360-361
        return (NO_KIND, EV_ACCEPT, key)
    return none


def classify(rows, filter_pid=0, filter_uid=-1, mntns=None):
    """classify_row over all rows, as the arrays igx_tcp_classify writes: tuple (n, 40) u8, kind,
    event (u8), key1 (u64 = tid)."""
    n = len(rows["probe"])
    ns = None if mntns is None else set(int(x) for x in mntns)
    tup, kind, ev = np.zeros((n, 40), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        k, e, key = classify_row(rows, i, filter_pid, filter_uid, ns)
        kind[i], ev[i] = k, e
        tup[i] = np.frombuffer(key, np.uint8)
    return {"tuple": tup, "kind": kind, "event": ev, "key1": rows["tid"].astype(np.uint64)}


# ---- the chained join over classified rows (the contract of igx_chain_join) ---------------------
def chain_join(key1, key2, kind, valid=None):
    """One batch.  Returns (emitted, live): emitted is a list of (take, pass) in stream order, live
    the ENTER rows still in map 1 and the PASS / HELD rows still in map 2, ascending."""
    m1, m2, emitted = {}, {}, []
    for i in range(len(kind)):
        if valid is not None and not valid[i]:
            continue
        k = int(kind[i])
        if k == ENTER:
            m1[int(key1[i])] = i                                    # :185
        elif k == PASS:
            if m1.pop(int(key1[i]), None) is not None:              # :203-205, :225
                m2[int(key2[i])] = i                                # :222
        elif k == ABORT:
            m1.pop(int(key1[i]), None)                              # :225
        elif k == TAKE:
            p = m2.pop(int(key2[i]), None)                          # :315, :327
            if p is not None:
                emitted.append((i, p))                              # :319-324
        elif k == DROP:
            m2.pop(int(key2[i]), None)                              # :327
        elif k == HELD:
            m2[int(key2[i])] = i
    return emitted, sorted(list(m1.values()) + list(m2.values()))


def chain_join_arrays(key1, key2, kind, valid=None):
    em, live = chain_join(key1, key2, kind, valid)
    cols = list(zip(*em)) if em else [(), ()]
    return np.array(cols[0], np.uint32), np.array(cols[1], np.uint32), np.array(live, np.uint32)


def chain_join_batches(key1, key2, kind, cuts, valid=None, join_fn=None):
    """The stream cut at `cuts` and joined batch by batch with the in-band carry: the live rows
    of the batch before go in front, in order, carried PASS rows as HELD.  Returns (emitted, live)
    in global row numbers."""
    join_fn = chain_join if join_fn is None else join_fn
    key1, key2, kind = np.asarray(key1), np.asarray(key2), np.asarray(kind)
    bounds = [0] + list(cuts) + [len(kind)]
    carry = np.zeros(0, np.int64)
    emitted = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        rows = np.concatenate([carry, np.arange(a, b, dtype=np.int64)])
        kd = kind[rows].copy()
        head = kd[:len(carry)]
        head[head == PASS] = HELD
        v = None if valid is None else np.asarray(valid)[rows]
        em, live = join_fn(key1[rows], key2[rows], kd, v)
        emitted += [(int(rows[t]), int(rows[p])) for t, p in em]
        carry = rows[np.array(live, np.int64)] if len(live) else np.zeros(0, np.int64)
    return emitted, [int(x) for x in carry]


def random_chain_stream(n, nthreads, ntuples, seed, p_kind=(0.22, 0.2, 0.04, 0.2, 0.06, 0.03), p_other=0.05):
    """n rows: ENTER / PASS / ABORT / TAKE / DROP / HELD with the given shares over nthreads thread
    ids and ntuples tuple ids; p_other of the rows get a kind that does not exist."""
    rng = np.random.default_rng(seed)
    t = (rng.choice(1 << 22, nthreads, replace=False).astype(np.uint64) << np.uint64(8)) | np.uint64(3)
    u = rng.choice(1 << 30, ntuples, replace=False).astype(np.uint64)
    key1, key2 = t[rng.integers(0, nthreads, n)], u[rng.integers(0, ntuples, n)]
    kind = rng.choice(6, n, p=np.asarray(p_kind, float) / sum(p_kind)).astype(np.uint8)
    kind[rng.random(n) < p_other] = rng.choice(np.array([6, 7, 200, 255], np.uint8))
    return key1, key2, kind


# ---- the gadget: the BPF programs row by row, with their two maps --------------------------------
def trace(rows, filter_pid=0, filter_uid=-1, mntns=None):
    """Every probe in row order with `sockets` and `tuplepid` as dicts.  Returns the events as
    (type, row, src): type 'connect' / 'accept' / 'close', row the emitting row (tuple, family,
    timestamp), src the row whose pid / uid / mntns / comm the event carries."""
    ns = None if mntns is None else set(int(x) for x in mntns)
    flt = (filter_pid, filter_uid, ns)
    sockets, tuplepid, out = {}, {}, []
    for i in range(len(rows["probe"])):
        p, fam, tid = int(rows["probe"][i]), int(rows["family"][i]), int(rows["tid"][i])
        if p == P_ENTER:
            if not filter_event(rows, i, *flt):
                sockets[tid] = i                                    # :185
        elif p == P_RETURN:
            if tid not in sockets:
                continue                                            # :203-205
            if int(rows["ret"][i]) == 0:
                ok, key = fill_tuple(rows, i, fam)                  # the row model: see k_tcptrace.h
                if ok:
                    tuplepid[key] = i                               # :215-222
            del sockets[tid]                                        # :225
        elif p == P_STATE:
            st = int(rows["state"][i])
            key = bytes(40)
            if st in (ESTABLISHED, CLOSE):
                ok, key = fill_tuple(rows, i, fam)
                if ok and st == ESTABLISHED:
                    if key not in tuplepid:
                        continue                                    # :316-317: no delete either
                    out.append(("connect", i, tuplepid[key]))       # :319-324
            tuplepid.pop(key, None)                                 # :327
        else:
            k, e, _ = classify_row(rows, i, *flt)
            if e:
                out.append(("accept" if e == EV_ACCEPT else "close", i, i))
    return out


def trace_via_join(rows, cuts=(), filter_pid=0, filter_uid=-1, mntns=None):
    """The same events through classify -> tuple ids -> chain_join_batches: the decomposition the
    device gadget uses."""
    c = classify(rows, filter_pid, filter_uid, mntns)
    ids = {}
    key2 = np.array([ids.setdefault(bytes(t), len(ids)) for t in c["tuple"]], np.uint64)
    em, _ = chain_join_batches(c["key1"], key2, c["kind"], cuts)
    ev = [("connect", t, p) for t, p in em]
    ev += [("accept" if e == EV_ACCEPT else "close", int(i), int(i)) for i, e in enumerate(c["event"]) if e]
    return sorted(ev, key=lambda x: x[1])


# ---- row builders ----------------------------------------------------------------------------------
def empty_rows(n):
    r = {f: np.zeros((n, 16) if f in ("saddr", "daddr") else n, DTYPES[f]) for f in FIELDS}
    r["ts"] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(1000)
    r["comm"] = np.zeros((n, 16), np.uint8)
    return r


def make_rows(specs):
    """specs: dicts of field -> value; saddr / daddr as bytes (padded to 16), comm as bytes."""
    r = empty_rows(len(specs))
    for i, s in enumerate(specs):
        for k, v in s.items():
            if k in ("saddr", "daddr", "comm"):
                b = bytes(v)
                r[k][i, :len(b)] = np.frombuffer(b, np.uint8)
            else:
                r[k][i] = v
    return r


def take_rows(rows, idx):
    return {k: v[np.asarray(idx, np.int64)] for k, v in rows.items()}


ADDR_PATTERNS = (bytes(16), b"\x0a\x00\x00\x01" + bytes(12), bytes(12) + b"\xde\xad\xbe\xef",
                 bytes(range(1, 17)))   # zero; word 0 only; garbage in bytes 12..15 only; all


def field_table():
    """The exhaustive small table of tests/sanitize/tcptrace_main.cpp, in its loop order: every
    probe with its ret / state cases, three families, and each of saddr (4 patterns), daddr (4),
    dport, sport, num zero or not: 12 x 3 x 128 = 4608 rows.  pid / uid / mntns cycle through a
    few values so that every filter passes some rows and drops others."""
    aux = [(P_ENTER, 0, 0), (P_RETURN, 0, 0), (P_RETURN, -111, 0), (P_CLOSE, 0, ESTABLISHED), (P_CLOSE, 0, SYN_SENT),
           (P_CLOSE, 0, SYN_RECV), (P_CLOSE, 0, NEW_SYN_RECV), (P_CLOSE, 0, CLOSE), (P_STATE, 0, ESTABLISHED),
           (P_STATE, 0, CLOSE), (P_STATE, 0, SYN_SENT), (P_ACCEPT, 0, 0)]
    specs = []
    for probe, ret, state in aux:
        for fam in (AF_INET, AF_INET6, 1):
            for sa in ADDR_PATTERNS:
                for da in ADDR_PATTERNS:
                    for bits in range(8):
                        j = len(specs)
                        specs.append(dict(probe=probe, ret=ret, state=state, family=fam, saddr=sa, daddr=da,
                                          dport=0x5000 if bits & 1 else 0, sport=0x1F90 if bits & 2 else 0,
                                          num=0x0050 if bits & 4 else 0, netns=4026531840 + j % 3,
                                          tid=100 + j % 7, pid=10 + j % 5, uid=j % 3, mntns=4026532000 + j % 11))
    return make_rows(specs)


def to_event(rows, ev, boot_to_wall_ns=0):
    """One element of trace() as the fields of the gadget's event (tracer.go:198-228): the tuple,
    family and timestamp of the emitting row, the task of the src row; ports in host order."""
    import socket
    typ, row, src = ev
    fam = int(rows["family"][row])
    key = classify_row(rows, row)[2]          # unfiltered: the filters never change a key
    v4 = fam == AF_INET
    ntop = (lambda b: socket.inet_ntop(socket.AF_INET, b[:4])) if v4 else (lambda b: socket.inet_ntop(socket.AF_INET6, b))
    comm = bytes(rows["comm"][src])
    return {"Operation": typ, "Timestamp": int(rows["ts"][row]) + boot_to_wall_ns, "MountNsID": int(rows["mntns"][src]),
            "Pid": int(rows["pid"][src]), "Comm": comm.split(b"\0")[0].decode(), "IPVersion": 4 if v4 else 6,
            "Saddr": ntop(key[0:16]), "Daddr": ntop(key[16:32]), "Sport": int.from_bytes(key[32:34], "big"),
            "Dport": int.from_bytes(key[34:36], "big")}
