"""gadgets.AdviseSeccompTracer over a synthetic node -- three containers, one of them started by
runc, one that makes no syscall, one detached mid-stream -- against the same flow over the
row-by-row restatement (tests/seccomp_ref.py): collectResult() byte for byte, Peek / Delete, and
the profile the names turn into."""
import json

import numpy as np
import pytest

from seccomp_ref import SeccompRef

pytestmark = pytest.mark.gpu

PRCTL, SECCOMP = 157, 317
INIT = b"runc:[2:INIT]"
WEB, DB, IDLE, HOST = 4026532201, 4026532202, 4026532203, 4026531840


def columns(rows):
    comm = np.zeros((len(rows), 16), np.uint8)
    for i, r in enumerate(rows):
        comm[i, :len(r[3])] = np.frombuffer(r[3], np.uint8)
    return (np.array([r[0] for r in rows], np.uint64), np.array([r[1] for r in rows], np.uint32),
            np.array([r[2] for r in rows], np.uint64), comm, np.array([r[4] if len(r) > 4 else 0 for r in rows], np.uint8))


def node_batches():
    """The node's sys_enter rows in three batches.  web is started by runc: its set-up calls come
    before prctl(PR_GET_PDEATHSIG) and must not show, nor the seccomp() and
    prctl(PR_SET_NO_NEW_PRIVS) after it; db's rows are the workload's own; idle makes none."""
    startup = [(WEB, 56, 0, INIT), (WEB, 165, 0, INIT), (WEB, 161, 0, INIT),          # clone, mount, chroot: before
               (WEB, PRCTL, 2, INIT),                                               # the gate
               (WEB, PRCTL, 38, INIT), (WEB, SECCOMP, 1, INIT),                     # excluded
               (WEB, 3, 0, INIT), (WEB, 59, 0, INIT)]                               # close, execve: recorded
    rng = np.random.default_rng(12)
    busy = [(int(rng.choice([WEB, DB, HOST])), int(rng.choice([0, 1, 3, 9, 202, 232, 257, 262])), 0, b"nginx")
            for _ in range(3000)]
    one = startup[:5] + busy[:1000] + [(DB, 60, 0, b"postgres", 1)]                 # a compat row: dropped
    two = startup[5:] + busy[1000:2000] + [(DB, 44, 0, b"postgres")]
    three = busy[2000:] + [(WEB, 499, 0, b"nginx"), (DB, 47, 0, b"postgres")]
    return one, two, three


def expected_json(result):
    """json.MarshalIndent(map[string][]string, "", "  ") for names that need no escaping."""
    return json.dumps(result, indent=2, sort_keys=True)


def test_collect_result_matches_the_reference_flow(igx):
    G, D = igx.gadgets, igx.columns.to_device
    names = importlib_names(igx)
    name_list = lambda v: sorted(names.get(i, "syscall%d" % i) for i in range(500) if v[i])   # noqa: E731
    t, ref = G.AdviseSeccompTracer(capacity=64), SeccompRef()
    try:
        web, db, idle, late = (G.SeccompContainer(n, m) for n, m in
                               (("web", WEB), ("db", DB), ("idle", IDLE), ("late", 4026532299)))
        for c in (web, db, idle, late):
            t.AttachContainer(c)
        want = {"web": None, "db": None, "idle": None, "late": None}
        one, two, three = node_batches()

        def feed(rows):
            cols = columns(rows)
            t.feed(*(D(c) for c in cols))
            ref.feed(*cols)

        feed(one)
        feed(two)
        t.DetachContainer(db)                                  # detached mid-stream: what it has so far
        want["db"] = name_list(ref.lookup(DB))
        assert t.Peek(DB) == want["db"] and "sendto" in want["db"] and "exit" not in want["db"]
        feed(three)
        t.DetachContainer(web)
        want["web"] = name_list(ref.lookup(WEB))
        t.DetachContainer(idle)                                # made no syscall: the error's text
        assert ref.lookup(IDLE) is None
        want["idle"] = ["no syscall found"]
        got = t.collectResult()                                # late was never detached: null
        assert got == expected_json(want)
        assert json.loads(got)["late"] is None
        assert "syscall499" in want["web"]                     # no table names 499
        for call in ("clone", "mount", "chroot", "seccomp", "prctl"):
            assert call not in want["web"]
        assert "execve" in want["web"] and "close" in want["web"]
        # the host's namespace was recorded too, though no container has it
        assert t.Peek(HOST) == name_list(ref.lookup(HOST))
        assert t.Peek(0) == []                                 # the blank value at key 0
        with pytest.raises(LookupError, match="^no syscall found$"):
            t.Peek(IDLE)
        t.Delete(WEB)
        with pytest.raises(LookupError, match="^no syscall found$"):
            t.Peek(WEB)
        assert t.collectResult() == got                        # results already taken stay
    finally:
        t.destroy()


def importlib_names(igx):
    import importlib
    return importlib.import_module(igx.__name__ + "._syscalls").X86_64


def test_callers_table_and_profile(igx):
    G, D = igx.gadgets, igx.columns.to_device
    t = G.AdviseSeccompTracer(capacity=8, goarch="arm64", names={0: "zero", 63: "read"})
    try:
        rows = [(5, 0, 0, b"app"), (5, 63, 0, b"app"), (5, 64, 0, b"app"),
                (5, 157, 2, INIT), (5, 167, 2, INIT), (5, 277, 0, INIT), (5, 157, 2, INIT)]   # arm64: prctl is 167
        t.feed(*(D(c) for c in columns(rows)[:4]))             # arm64 has no compat column
        names = t.Peek(5)
        assert names == ["read", "syscall157", "syscall64", "zero"]
        prof = G.go_marshal(G.SyscallNamesToLinuxSeccomp(names, "arm64"), indent="  ", sort_maps=False)
        assert prof == """{
  "defaultAction": "SCMP_ACT_ERRNO",
  "architectures": [
    "SCMP_ARCH_ARM",
    "SCMP_ARCH_AARCH64"
  ],
  "syscalls": [
    {
      "names": [
        "read",
        "syscall157",
        "syscall64",
        "zero"
      ],
      "action": "SCMP_ACT_ALLOW"
    }
  ]
}"""
    finally:
        t.destroy()
