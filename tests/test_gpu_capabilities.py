"""gadgets.TraceCapabilitiesTracer on the device against tests/capabilities_ref.py, every field of
every event: one stream of about 50 000 probe rows over 200 threads and 8 mount namespaces under
each configuration (defaults, --unique, audit-only off, a 4.19 kernel, a mount namespace filter,
targ_pid, my_pid, the arm64 skip numbers), in one batch and again in 5; then the two traps: a
cap_capable exit with no syscall entry against one with syscall 0 pending, and a --unique
CAP_ENTER admitted in one batch whose exit comes in the next.

The floors on the event counts were checked on the restatement alone."""
import functools

import numpy as np
import pytest

import capabilities_ref as R

pytestmark = pytest.mark.gpu

N_ROWS, SEED = 50_000, 7


@functools.lru_cache(maxsize=None)
def _stream():
    ev = R.random_stream(N_ROWS, SEED)
    return ev


def _targ(ev):
    """The pid with the most rows."""
    pids, cnt = np.unique(ev["pid_tgid"] >> np.uint64(32), return_counts=True)
    return int(pids[np.argmax(cnt)])


# name -> (tracer arguments, restatement arguments, floor on the events)
CONFIGS = {
    "defaults": ({}, {}, 2000),
    "unique": ({"Unique": True}, {"unique": True}, 40),
    "audit-off": ({"AuditOnly": False}, {"audit_only": False}, 3000),
    "kernel-4.19": ({"kernel_version": (4, 19, 0)}, {"version": R.kernel_version(4, 19, 0)}, 2000),
    "mntns-filter": ({"mntns_filter": [4026531841, 4026531844, 4026531847]},
                     {"mntns_filter": [4026531841, 4026531844, 4026531847]}, 500),
    "targ-pid": ({"targ_pid": "TARG"}, {"targ_pid": "TARG"}, 10),
    "my-pid": ({"my_pid": "TARG"}, {"my_pid": "TARG"}, 2000),
    "arm64": ({"goarch": "arm64"}, {"goarch": "arm64"}, 2000),
    "unique-audit-off-4.19": ({"Unique": True, "AuditOnly": False, "kernel_version": (4, 19, 0)},
                              {"unique": True, "audit_only": False, "version": R.kernel_version(4, 19, 0)}, 40),
}


def _args(d, ev):
    return {k: (_targ(ev) if v == "TARG" else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _reference(name):
    ev = _stream()
    kw = _args(CONFIGS[name][1], ev)
    m = R.Machine(**kw)
    raw = m.feed(ev)
    return raw, kw.get("version", R.kernel_version(5, 15, 0)), len(m.start) + len(m.current_syscall)


def _compare(igx, got, raw, version, names):
    G = igx.gadgets
    assert len(got) == len(raw)
    for e, r in zip(got, raw):
        d = R.to_event(r, version, G.CAPABILITY_NAMES, names)
        assert {k: getattr(e, k) for k in d} == d


def _feed(igx, tr, ev, bounds):
    H = igx.columns
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        out += tr.feed({k: H.to_device(v[lo:hi]) for k, v in ev.items()})
    return out


@pytest.mark.parametrize("batches", [1, 5])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_stream(igx, name, batches):
    ev = _stream()
    raw, version, pending = _reference(name)
    assert len(raw) >= CONFIGS[name][2] and pending >= 10
    n = len(ev["kind"])
    cuts = [] if batches == 1 else sorted(int(x) for x in np.random.default_rng(11).choice(np.arange(1, n), batches - 1,
                                                                                         replace=False))
    tr = igx.gadgets.TraceCapabilitiesTracer(**_args(CONFIGS[name][0], ev))
    try:
        got = _feed(igx, tr, ev, [0] + cuts + [n])
        _compare(igx, got, raw, version, tr.names)
        assert tr.pending == pending                    # the entries left in `start` and `current_syscall`
        if name == "defaults":
            # the stream exercises what it is meant to: absent and present syscalls, syscall 0, denials, unknown caps
            sys = [e.Syscall for e in got]
            assert sys.count("") > 100 and sys.count("read") > 50 and sys.count("socket") > 50
            assert sum(e.Verdict == "Deny" for e in got) > 300 and any(e.CapName == "UNKNOWN (41)" for e in got)
    finally:
        tr.destroy()


def _rows(seq):
    n = len(seq)
    ev = {"kind": np.array([s[0] for s in seq], np.uint8),
          "pid_tgid": np.array([(100 << 32) | s[1] for s in seq], np.uint64),
          "mntns": np.full(n, 4026531840, np.uint64), "ts": np.arange(n, dtype=np.uint64) + np.uint64(1000),
          "nr": np.array([s[2] for s in seq], np.uint64), "cap": np.array([s[3] for s in seq], np.int32),
          "cap_opt": np.zeros(n, np.int32), "cred_is_real": np.ones(n, np.uint8),
          "current_userns": np.full(n, 1, np.uint64), "target_userns": np.full(n, 2, np.uint64),
          "cap_effective": np.arange(n, dtype=np.uint64) + np.uint64(1), "ret": np.zeros(n, np.int32),
          "uid": np.zeros(n, np.uint32), "comm": np.zeros((n, 16), np.uint8)}
    return ev


@pytest.mark.parametrize("cut", [None, 2, 3])
def test_absent_syscall_is_not_syscall_zero(igx, cut):
    """Thread 1 is inside read (nr 0) when cap_capable returns; thread 2 has no syscall entry.  The
    gathered B row of thread 2 is a zero row, which must not read as syscall 0."""
    E, X, S = R.CAP_ENTER, R.CAP_EXIT, R.SYS_ENTER
    ev = _rows([(S, 1, 0, 0), (E, 1, 0, 21), (E, 2, 0, 21), (X, 1, 0, 0), (X, 2, 0, 0)])
    raw = R.Machine().feed(ev)
    assert [r["syscall"] for r in raw] == [0, -1]
    tr = igx.gadgets.TraceCapabilitiesTracer()
    try:
        got = _feed(igx, tr, ev, [0, 5] if cut is None else [0, cut, 5])
        assert [e.Syscall for e in got] == ["read", ""]
        _compare(igx, got, raw, R.kernel_version(5, 15, 0), tr.names)
    finally:
        tr.destroy()


def test_unique_admitted_row_straddles_a_batch(igx):
    """--unique: the CAP_ENTER of (21, mntns) is admitted in batch 1 and its exit comes in batch 2.
    The carried row is in `seen` already and must not meet the gate again; the second CAP_ENTER of
    the same key in batch 2 must be dropped and leave the pending entry untouched."""
    E, X = R.CAP_ENTER, R.CAP_EXIT
    ev = _rows([(E, 1, 0, 21), (E, 2, 0, 12), (E, 1, 0, 21), (X, 1, 0, 0), (X, 2, 0, 0), (E, 2, 0, 12), (X, 2, 0, 0)])
    raw = R.Machine(unique=True).feed(ev)
    assert [(r["pid"], r["cap"], r["cap_effective"]) for r in raw] == [(100, 21, 1), (100, 12, 2)]
    for bounds in ([0, 2, 7], [0, 1, 2, 3, 4, 5, 6, 7], [0, 7]):
        tr = igx.gadgets.TraceCapabilitiesTracer(Unique=True)
        try:
            got = _feed(igx, tr, ev, bounds)
            assert [(e.Cap, e.Caps) for e in got] == [(21, 1), (12, 2)], bounds
            _compare(igx, got, raw, R.kernel_version(5, 15, 0), tr.names)
            assert tr.pending == 0
        finally:
            tr.destroy()
