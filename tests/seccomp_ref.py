"""ig_seccomp_e (pkg/gadgets/advise/seccomp/tracer/bpf/seccomp.bpf.c:67-139) restated row by row,
exactly as the BPF program is written: a dict of 501-byte values keyed by mount namespace, with
the blank value the tracer installs at key 0 (tracer.go:77), Lookup and Delete.  The reference's
max_entries is not modelled (a dict does not fill up).  Test infrastructure only."""

SYSCALLS_COUNT = 500
VALUE_SIZE = SYSCALLS_COUNT + 1
PR_GET_PDEATHSIG = 2
PR_SET_NO_NEW_PRIVS = 38
NR_X86_64 = (157, 317)   # __NR_prctl, __NR_seccomp
NR_ARM64 = (167, 277)


class SeccompRef:
    def __init__(self, nr_prctl=NR_X86_64[0], nr_seccomp=NR_X86_64[1]):
        self.nr_prctl, self.nr_seccomp = nr_prctl, nr_seccomp
        self.map = {0: bytearray(VALUE_SIZE)}

    def row(self, mntns, id, arg0, comm, compat=0):
        """One sys_enter.  comm: 16 bytes (shorter is zero-padded)."""
        comm = bytes(comm).ljust(16, b"\0")
        if compat:                                   # :78-80
            return
        if id >= SYSCALLS_COUNT:                     # :83-84 (id is unsigned)
            return
        is_runc = comm[0:4] == b"runc"               # :88
        if mntns == 0:                               # :91-93
            return
        bitmap = self.map.get(mntns)
        if bitmap is None:                           # :96-106
            bitmap = self.map[mntns] = bytearray(self.map[0])
        if is_runc:
            if bitmap[SYSCALLS_COUNT] == 0:          # :117-124
                if id == self.nr_prctl and arg0 == PR_GET_PDEATHSIG:
                    bitmap[SYSCALLS_COUNT] = 1
                return
            if (id == self.nr_prctl and arg0 == PR_SET_NO_NEW_PRIVS) or id == self.nr_seccomp:   # :129-132
                return
        bitmap[id] = 1                               # :136

    def feed(self, mntns, id, arg0, comm, compat=None, valid=None):
        """Rows in stream order; rows with valid[i] == 0 never reached the program."""
        aslist = lambda c: c.tolist() if hasattr(c, "tolist") else list(c)   # noqa: E731  (numpy columns)
        mntns, id, arg0 = aslist(mntns), aslist(id), aslist(arg0)
        compat = [0] * len(mntns) if compat is None else aslist(compat)
        for i in range(len(mntns)):
            if valid is not None and not valid[i]:
                continue
            self.row(mntns[i], id[i], arg0[i], bytes(comm[i]), compat[i])

    def lookup(self, mntns):
        """LookupBytes: the 501 bytes, or None."""
        v = self.map.get(mntns)
        return None if v is None else bytes(v)

    def delete(self, mntns):
        """Delete of a container's namespace; the blank value at key 0 is the tracer's own and
        no caller deletes it."""
        if mntns != 0:
            self.map.pop(mntns, None)
