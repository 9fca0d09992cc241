"""Host restatements for profile cpu (paths under the reference root
pkg/gadgets/profile/cpu): the row interner's contract as a dict, findKernelSymbol line by line
(tracer/tracer.go:184-208), readKernelSymbols (:139-177), and the probe (tracer/bpf/
profile.bpf.c:60-114) plus collectResult / getReport (tracer.go:210-322) over plain Python
values.  The device tests compare with these bit for bit."""
import json

NO_COL = 0xFFFFFFFF
UNKNOWN = "[unknown]"


class DictInterner:
    """include/igx.h, igx_intern: ids by first appearance in the stream."""

    def __init__(self):
        self.ids = {}
        self.rows = []

    def add(self, rows, valid=None):
        """rows: iterable of bytes.  Returns the ids (NO_COL where valid is 0)."""
        out = []
        for i, r in enumerate(rows):
            if valid is not None and not valid[i]:
                out.append(NO_COL)
                continue
            r = bytes(r)
            if r not in self.ids:
                self.ids[r] = len(self.rows)
                self.rows.append(r)
            out.append(self.ids[r])
        return out


def find_kernel_symbol(addrs, ip):
    """findKernelSymbol: the index of the symbol, or NO_COL for "[unknown]"."""
    end = len(addrs) - 1
    addr = 0
    start = 0
    while start < end:
        mid = start + (end - start + 1) // 2
        addr = addrs[mid]
        if addr <= ip:
            start = mid
        else:
            end = mid - 1
    if start == end and addrs[start] <= addr:
        return start
    return NO_COL


def read_kernel_symbols(text):
    """readKernelSymbols over the text of /proc/kallsyms: [(addr, name)]."""
    out = []
    for line in text.splitlines():
        fields = line.split()
        if len(fields) < 3:
            continue
        # strconv.ParseUint(s, 16, 64): hex digits only (no sign, prefix or underscore), 64 bits
        if not fields[0] or any(c not in "0123456789abcdefABCDEF" for c in fields[0]) or int(fields[0], 16) >> 64:
            raise ValueError(f'strconv.ParseUint: parsing "{fields[0]}": invalid syntax')
        out.append((int(fields[0], 16), fields[2]))
    return out


def from_c_string(b):
    b = bytes(b)
    i = b.find(b"\0")
    return (b if i < 0 else b[:i]).decode("utf-8", "replace")


class ProfileCpuRef:
    """The probe over samples one at a time, the counts map as a dict (insertion order is the
    first-occurrence order that replaces the BPF map's hash order), one stack map for both
    stacks with kernel rows added before user rows in each feed."""

    def __init__(self, user_stack_only=False, kernel_stack_only=False, include_idle=False, kallsyms=()):
        self.user_only, self.kernel_only, self.idle = user_stack_only, kernel_stack_only, include_idle
        self.syms = list(kallsyms)
        self.stacks = DictInterner()
        self.counts = {}

    def feed(self, pid, tid, mntns, comm, ip, kstack, kstatus, ustack, ustatus):
        """Columns as Python lists; kstack / ustack: one bytes row per sample (the frames as
        little-endian u64, zero-padded to the depth)."""
        n = len(pid)
        keep = [self.idle or tid[i] != 0 for i in range(n)]
        kvalid = [keep[i] and not self.user_only and kstatus[i] >= 0 for i in range(n)]
        uvalid = [keep[i] and not self.kernel_only and ustatus[i] >= 0 for i in range(n)]
        kid = self.stacks.add(kstack, kvalid)
        uid = self.stacks.add(ustack, uvalid)
        for i in range(n):
            if not keep[i]:
                continue
            ks = -1 if self.user_only else (kstatus[i] if kstatus[i] < 0 else kid[i])
            us = -1 if self.kernel_only else (ustatus[i] if ustatus[i] < 0 else uid[i])
            kip = ip[i] if ks >= 0 and ip[i] >> 63 else 0
            key = (kip, mntns[i], pid[i], us, ks, bytes(comm[i]))
            self.counts[key] = self.counts.get(key, 0) + 1

    def reports(self):
        """collectResult: ascending count, ties by first occurrence; one dict per report."""
        order = sorted(enumerate(self.counts.items()), key=lambda e: (e[1][1], e[0]))
        addrs = [a for a, _ in self.syms]
        resolved = {}     # kernel stack id -> names (getReport resolves per report; the same stack gives the same names)
        out = []
        for _, ((kip, mntns, pid, us, ks, name), count) in order:
            ustack, kstack = [], []
            if us >= 0:
                row = self.stacks.rows[us]
                for o in range(0, len(row), 8):
                    if int.from_bytes(row[o:o + 8], "little") == 0:
                        break
                    ustack.append(UNKNOWN)
            if ks >= 0 and ks in resolved:
                kstack = list(resolved[ks])
            elif ks >= 0:
                row = self.stacks.rows[ks]
                for o in range(0, len(row), 8):
                    a = int.from_bytes(row[o:o + 8], "little")
                    if a == 0:
                        break
                    j = find_kernel_symbol(addrs, a)
                    kstack.append(UNKNOWN if j == NO_COL else self.syms[j][1])
                resolved[ks] = list(kstack)
            out.append({"Comm": from_c_string(name), "Pid": pid, "UserStack": ustack, "KernelStack": kstack,
                        "Count": count, "MntnsID": mntns})
        return out

    def stop(self):
        """json.Marshal([]Report) with the omitempty tags of types/types.go:27-37 (CommonData is
        empty without an enricher and MntnsID is `json:"-"`)."""
        out = []
        for r in self.reports():
            d = {}
            for k, j in (("Comm", "comm"), ("Pid", "pid"), ("UserStack", "userStack"),
                         ("KernelStack", "kernelStack"), ("Count", "count")):
                if r[k]:
                    d[j] = r[k]
            out.append(d)
        return json.dumps(out, separators=(",", ":"), ensure_ascii=False)


# findKernelSymbol by hand: (table, ip, expected index), worked through the loop on paper.
KSYM_HAND_CASES = [
    ([], 0x1234, NO_COL),                                   # len 0: start == end never holds
    ([0], 5, 0),                                            # len 1 resolves only at address 0 ...
    ([0x1000], 0x1004, NO_COL),                             # ... since addr stays 0
    ([0x1000, 0x2000], 0x1004, 0),
    ([0x1000, 0x2000], 0x2004, 1),
    ([0x1000, 0x2000], 0x10, 0),                            # below the first symbol: still symbol 0
    ([0x1000, 0x2000, 0x3000], 0x2000, 1),                  # ip equal to an address
    ([0x1000, 0x2000, 0x3000], 0x2FFF, 1),
    ([0x1000, 0x2000, 0x3000], 0xFFFFFFFFFFFFFFFF, 2),
    ([0x1000, 0x2000, 0x2000, 0x3000], 0x2000, 2),          # duplicates: the last of them
    ([0x9000, 0x1000, 0x8000], 0x500, NO_COL),              # unsorted: sym[0] > the last address probed
    ([0x5000, 0x1000], 0x2000, 1),                          # unsorted, resolves
]
