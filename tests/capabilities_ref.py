"""Sequential restatement of trace capabilities: capable.bpf.c probe by probe over Python dicts
(`start`, `current_syscall`, `seen`, the mount namespace filter), then tracer.go:257-318 on each
cap_event.  A helper for the tests of gadgets.TraceCapabilitiesTracer, not a test module."""
import numpy as np

CAP_ENTER, CAP_EXIT, SYS_ENTER, SYS_EXIT = 0, 1, 2, 3
SKIP = {"amd64": (60, 231, 15), "arm64": (93, 94, 139)}       # capable.bpf.c:202-212
COLS = ("kind", "pid_tgid", "mntns", "ts", "nr", "cap", "cap_opt", "cred_is_real", "current_userns",
        "target_userns", "cap_effective", "ret", "uid", "comm")


def kernel_version(a, b, c):
    return (a << 16) + (b << 8) + min(c, 255)


class Machine:
    """The BPF side.  The maps live on between feeds, as the kernel's do."""

    def __init__(self, unique=False, audit_only=True, version=kernel_version(5, 15, 0), mntns_filter=None, my_pid=-1,
                 targ_pid=-1, goarch="amd64"):
        self.unique, self.audit_only, self.version = unique, audit_only, version
        self.filter = None if mntns_filter is None else set(int(x) for x in mntns_filter)
        self.my_pid, self.targ_pid, self.skip = my_pid & 0xFFFFFFFF, targ_pid, SKIP[goarch]
        self.start, self.current_syscall, self.seen = {}, {}, set()

    def feed(self, ev):
        """ev: {column: numpy array}; returns the cap_event dicts the kretprobe outputs, in order."""
        out = []
        for i in range(len(ev["kind"])):
            kind, pid_tgid, mntns = int(ev["kind"][i]), int(ev["pid_tgid"][i]), int(ev["mntns"][i])
            if kind == CAP_ENTER:                                            # :87-150
                if self.filter is not None and mntns not in self.filter:
                    continue
                if not ev["cred_is_real"][i]:
                    continue
                pid = pid_tgid >> 32
                if pid == self.my_pid:
                    continue
                if self.targ_pid != -1 and (self.targ_pid & 0xFFFFFFFF) != pid:
                    continue
                cap, cap_opt = int(ev["cap"][i]), int(ev["cap_opt"][i])
                if self.audit_only:
                    if self.version >= kernel_version(5, 1, 0):
                        if cap_opt & 2:
                            continue
                    elif not cap_opt:
                        continue
                if self.unique:
                    if (cap, mntns) in self.seen:
                        continue
                    self.seen.add((cap, mntns))
                self.start[pid_tgid] = {"current_userns": int(ev["current_userns"][i]),
                                        "target_userns": int(ev["target_userns"][i]),
                                        "cap_effective": int(ev["cap_effective"][i]), "cap": cap, "cap_opt": cap_opt}
            elif kind == CAP_EXIT:                                           # :152-196
                ap = self.start.get(pid_tgid)
                if ap is None:
                    continue
                e = dict(ap, pid=pid_tgid >> 32, uid=int(ev["uid"][i]), mntnsid=mntns, task=ev["comm"][i].tobytes(),
                         ret=int(ev["ret"][i]), timestamp=int(ev["ts"][i]),
                         syscall=self.current_syscall.get(pid_tgid, -1))
                out.append(e)
                del self.start[pid_tgid]
            elif kind == SYS_ENTER:                                          # :220-240
                if self.filter is not None and mntns not in self.filter:
                    continue
                nr = int(ev["nr"][i])
                snr = (nr & 0xFFFFFFFF) - ((nr & 0x80000000) << 1)           # skip_exit_probe(int nr)
                if snr not in self.skip:
                    self.current_syscall[pid_tgid] = nr
            elif kind == SYS_EXIT:                                           # :242-248
                self.current_syscall.pop(pid_tgid, None)
        return out


def to_event(e, version, cap_names, syscall_names, boot_to_wall_ns=0):
    """tracer.go:257-318 as a dict keyed by the types.Event field names."""
    cap = e["cap"]
    name = cap_names[cap] if 0 <= cap < len(cap_names) else "UNKNOWN (%d)" % cap
    if version >= kernel_version(5, 1, 0):
        audit = 1 if (e["cap_opt"] & 0b10) == 0 else 0
        inset = bool(e["cap_opt"] & 0b100)
    else:
        audit, inset = e["cap_opt"], None
    s32 = (e["syscall"] & 0xFFFFFFFF) - ((e["syscall"] & 0x80000000) << 1)
    task = e["task"]
    task = task[:task.index(b"\0")] if b"\0" in task else task
    return {"Timestamp": e["timestamp"] + boot_to_wall_ns, "MountNsID": e["mntnsid"], "Pid": e["pid"],
            "Comm": task.decode("utf-8", "replace"), "Syscall": syscall_names.get(s32, "") if s32 >= 0 else "",
            "UID": e["uid"], "Cap": cap, "CapName": name, "Audit": audit, "Verdict": "Allow" if e["ret"] == 0 else "Deny",
            "InsetID": inset, "TargetUserNs": e["target_userns"], "CurrentUserNs": e["current_userns"],
            "Caps": e["cap_effective"],
            "CapsNames": [cap_names[i].lower() for i in range(len(cap_names)) if (1 << i) & e["cap_effective"]]}


def random_stream(n, seed, nthreads=200, nns=8, p_cap=0.06):
    """About n probe rows over nthreads threads in nns mount namespaces, each thread a plausible
    sequence: sys_enter, a few cap_capable enter / exit pairs, sys_exit -- with planted irregularities:
    lost exits and entries, overridden credentials, NOAUDIT checks, the syscalls sys_enter skips, and
    cap_capable outside any syscall.  The threads' sequences are interleaved at random."""
    rng = np.random.default_rng(seed)
    tid = rng.choice(np.arange(1000, 1000 + 4 * nthreads), nthreads, replace=False).astype(np.uint64)
    pid_tgid = ((tid // np.uint64(3) + np.uint64(100)) << np.uint64(32)) | tid
    ns_of = np.uint64(4026531840) + rng.integers(0, nns, nthreads).astype(np.uint64)
    uid_of = rng.choice(np.array([0, 1000, 65534], np.uint32), nthreads)
    comms = [b"runc:[2:INIT]", b"nginx", b"ping", b"systemd-journal", b"sixteen-byte-nam"]
    comm_of = rng.integers(0, len(comms), nthreads)
    nrs = np.array([0, 1, 2, 41, 49, 105, 165, 59, 60, 231, 15, 93, 94, 139, 999, 0xFFFFFFFFFFFFFFFF], np.uint64)
    rows = []                                              # (thread, kind, nr, cap, cap_opt, real, ret)
    per = max(1, n // nthreads)
    for t in range(nthreads):
        k = 0
        while k < per:
            nr = int(nrs[rng.integers(0, len(nrs))])
            if rng.random() > 0.03:                        # a lost sys_enter now and then
                rows.append((t, SYS_ENTER, nr, 0, 0, 1, 0))
                k += 1
            while rng.random() < p_cap * 4:
                cap = int(rng.choice([0, 1, 2, 7, 12, 13, 21, 38, 39, 40, 41, 63]))
                opt = int(rng.choice([0, 0, 1, 2, 4, 5, 6]))
                if rng.random() > 0.05:
                    rows.append((t, CAP_ENTER, nr, cap, opt, int(rng.random() > 0.1), 0))
                    k += 1
                if rng.random() > 0.05:
                    rows.append((t, CAP_EXIT, nr, 0, 0, 1, int(rng.choice([0, 0, -1]))))
                    k += 1
            if rng.random() > 0.1:                         # exit and friends never return; others are lost
                rows.append((t, SYS_EXIT, nr, 0, 0, 1, 0))
                k += 1
    # interleave: keep each thread's order, draw the next thread at random
    order = rng.permutation(np.repeat(np.arange(nthreads), np.bincount([r[0] for r in rows], minlength=nthreads)))
    by_thread = [[] for _ in range(nthreads)]
    for r in rows:
        by_thread[r[0]].append(r)
    nxt = [0] * nthreads
    seq = []
    for t in order:
        seq.append(by_thread[t][nxt[t]])
        nxt[t] += 1
    m = len(seq)
    th = np.array([r[0] for r in seq])
    comm = np.zeros((m, 16), np.uint8)
    for i, t in enumerate(th):
        b = comms[comm_of[t]]
        comm[i, :len(b)] = np.frombuffer(b, np.uint8)
    return {"kind": np.array([r[1] for r in seq], np.uint8), "pid_tgid": pid_tgid[th], "mntns": ns_of[th],
            "ts": np.cumsum(rng.integers(1, 4000, m)).astype(np.uint64) + np.uint64(10 ** 12),
            "nr": np.array([r[2] for r in seq], np.uint64), "cap": np.array([r[3] for r in seq], np.int32),
            "cap_opt": np.array([r[4] for r in seq], np.int32), "cred_is_real": np.array([r[5] for r in seq], np.uint8),
            "current_userns": np.uint64(4026531837) + (th % 3).astype(np.uint64),
            "target_userns": np.uint64(4026531837) + (th % 2).astype(np.uint64),
            "cap_effective": rng.choice(np.array([0, 0x3FFFFFFFFF, 0x1FFFFFFFFFF, 0xA80425FB, 0xFFFFFFFFFFFFFFFF],
                                                 np.uint64), nthreads)[th],
            "ret": np.array([r[6] for r in seq], np.int32), "uid": uid_of[th], "comm": comm}
