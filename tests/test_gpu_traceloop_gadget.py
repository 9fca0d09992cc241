"""gadgets.TraceloopTracer fed raw samples for three containers: a write with a cont, an openat
whose string cont holds a non-printable byte, a failed cont, an exit_group, an orphan exit, and an
unknown enter number (which must fail the read).  ReadAll() -- one device join over every
container -- equals three Read()s, both equal the events built from tests/traceloop_ref.py, and the
rendered table carries the params / ret text of types.go:54-73."""
import numpy as np
import pytest

import traceloop_ref as R
from test_traceloop_host import cont_sample, sys_sample

pytestmark = pytest.mark.gpu

DECL = {"write": ["fd", "buf", "count"], "openat": ["dfd", "filename", "flags", "mode"],
        "exit_group": ["error_code"], "read": ["fd", "buf", "count"], "close": ["fd"]}
WALL = 1_700_000_000_000_000_000
MNTNS = {"c1": 4026532001, "c2": 4026532002, "c3": 4026532003}


def samples():
    """Per container, in ring order.  Timestamp 500 is used in all three containers."""
    c1 = [sys_sample(500, 1500, 0, 1, 10, cpu=1, comm=b"cat", args=(1, 0x7FFF0000, 6, 0, 0, 0), cont_nr=1),
          cont_sample(500, 1, b"hello\n", length=6),
          b"\0" * 64,                                                           # a sample of another size
          sys_sample(500, 1501, 1, 1, 10, cpu=1, comm=b"cat", args=(6, 0, 0, 0, 0, 0)),
          sys_sample(700, 1700, 0, 231, 10, cpu=1, comm=b"cat", args=(0, 0, 0, 0, 0, 0))]
    c2 = [sys_sample(500, 1400, 0, 257, 20, cpu=2, comm=b"sh", args=((1 << 64) - 100, 0x5000, 0, 0, 0, 0), cont_nr=1),
          cont_sample(500, 1, b"/tmp/a\x01b\xff"),
          sys_sample(500, 1401, 1, 257, 20, cpu=2, comm=b"sh", args=((1 << 64) - 2, 0, 0, 0, 0, 0)),
          sys_sample(600, 1600, 0, 0, 20, cpu=3, comm=b"sh", args=(3, 0x6000, 128, 0, 0, 0)),   # a read never finished
          sys_sample(650, 1650, 1, 3, 21, cpu=3, comm=b"sh")]                                   # an orphan exit (close)
    c3 = [sys_sample(500, 1450, 0, 1, 30, comm=b"dd", args=(2, 0x9000, 4, 0, 0, 0)),
          cont_sample(500, 1, b"", length=4, failed=1),
          sys_sample(500, 1451, 1, 1, 30, comm=b"dd", args=((1 << 64) - 14, 0, 0, 0, 0, 0))]
    return {"c1": c1, "c2": c2, "c3": c3}


def tracer(igx, **kw):
    t = igx.gadgets.TraceloopTracer(DECL, boot_to_wall_ns=WALL, **kw)
    for c, mn in MNTNS.items():
        t.Attach(c, mn)
    for c, s in samples().items():
        t.feed(c, s)
    return t


def ref_events(igx, cid, have_boot_ns=True):
    G = igx.gadgets
    s, c = G.traceloop_decode(samples()[cid])
    out = R.join(s["mono_ts"], s["boot_ts"] if have_boot_ns else s["mono_ts"], s["typ"], s["id"], s["pid"],
                 c_mono_ts=c["mono_ts"], c_index=c["index"])
    from importlib import import_module
    names = import_module("inspektor-gadget_amd._syscalls").X86_64
    return G.traceloop_events(s, c, *out, names, DECL, MNTNS[cid], have_boot_ns, WALL)


def test_read_all_equals_reads_equals_reference(igx):
    every = tracer(igx).ReadAll()
    one = tracer(igx)
    for cid in MNTNS:
        want = ref_events(igx, cid)
        assert every[cid] == want, cid
        assert one.Read(cid) == want, cid
        assert one.Read(cid) == []                       # a read consumes what it saw
    w, x = every["c1"]
    assert (w.Syscall, w.Timestamp, w.CPU, w.Pid, w.Comm, w.MountNsID, w.Retval) == ("write", WALL + 1500, 1, 10, "cat",
                                                                                     MNTNS["c1"], 6)
    assert [(p.Name, p.Value) for p in w.Parameters] == [("fd", "1"), ("buf", '"hello\\n"'), ("count", "6")]
    assert (x.Syscall, x.Retval, [(p.Name, p.Value) for p in x.Parameters]) == ("exit_group", 0, [("error_code", "0")])
    o, r, e = every["c2"]
    assert o.Syscall == "openat" and o.Retval == -2
    assert [(p.Name, p.Value) for p in o.Parameters] == [("dfd", str((1 << 64) - 100)), ("filename", '"/tmp/a\\x01b\\xff"'),
                                                         ("flags", "0"), ("mode", "0")]
    assert (r.Syscall, r.Parameters, r.Retval) == ("read", [], 0)          # incomplete enter
    assert (e.Syscall, e.Parameters, e.Pid) == ("close", [], 21)           # incomplete exit
    (d,) = every["c3"]
    assert d.Parameters[1].Value == '"(Failed to dereference pointer)"' and d.Retval == -14


def test_rendered_table(igx):
    every = tracer(igx).ReadAll()
    lines = igx.gadgets.traceloop_render(every["c1"] + every["c2"]).split("\n")
    assert lines[0].split() == ["CPU", "PID", "COMM", "SYSCALL", "PARAMS", "RET"]
    assert 'fd=1, buf="hello\\n", count=6' in lines[1] and lines[1].rstrip().endswith(" 6")
    assert "error_code=0" in lines[2] and lines[2].rstrip().endswith(" X")
    assert "openat" in lines[3] and lines[3].rstrip().endswith("-2")


def test_without_boot_timestamps(igx):
    t = tracer(igx, have_boot_ns=False)
    for cid in MNTNS:
        ev = t.Read(cid)
        assert ev == ref_events(igx, cid, have_boot_ns=False) and all(e.Timestamp == 0 for e in ev)


def test_unknown_enter_number_fails_the_read(igx):
    t = tracer(igx)
    t.feed("c3", [sys_sample(900, 1900, 0, 499, 30)])          # no such syscall on x86_64
    with pytest.raises(LookupError):
        t.Read("c3")
    with pytest.raises(LookupError):
        t.ReadAll()
    # a named syscall without a declaration fails too; an unnamed exit is only skipped
    t = tracer(igx)
    t.feed("c1", [sys_sample(900, 1900, 0, 39, 10)])            # getpid: not in DECL
    with pytest.raises(LookupError):
        t.Read("c1")
    t = tracer(igx)
    t.feed("c1", [sys_sample(900, 1900, 1, 499, 10)])
    assert len(t.Read("c1")) == 2


def test_attach_detach_delete(igx):
    t = tracer(igx)
    t.Detach(MNTNS["c2"])
    t.feed("c2", [sys_sample(950, 1950, 1, 3, 21)])             # not recorded any more
    assert len(t.Read("c2")) == 3
    t.Delete("c2")
    with pytest.raises(LookupError):
        t.Read("c2")
    with pytest.raises(LookupError):
        t.Delete("c2")
    with pytest.raises(LookupError):
        t.Detach(12345)
    assert sorted(t.ReadAll()) == ["c1", "c3"]
