"""The host half of the traceloop gadget: go_quote (strconv.Quote restated), parseSyscall and
relateSyscallName (syscall_helpers.go:81-167), the raw sample decoder (tracer.go:272-348 over
traceloop.h:34-55) and the params / ret extractors (types.go:54-73).  No GPU."""
import struct

import numpy as np
import pytest


@pytest.fixture(scope="module")
def G(igx):
    return igx.gadgets


def test_go_quote(G):
    q = G.go_quote
    assert q(b'a"b\\c\n\t\x00\x7f') == '"a\\"b\\\\c\\n\\t\\x00\\x7f"'
    assert q(b"\xff") == '"\\xff"'
    assert q(" ") == '"\\u00a0"'
    assert q("​") == '"\\u200b"'
    assert q("\U000e0001") == '"\\U000e0001"'
    assert q("é") == '"é"' and q("\U0001f600") == '"\U0001f600"'
    assert q(b"\x07\x08\x0c\r\x0b\x1b") == '"\\a\\b\\f\\r\\v\\x1b"'
    # every byte of an invalid sequence on its own: a truncated rune, an overlong form, a surrogate
    assert q(b"\xe2\x82") == '"\\xe2\\x82"'
    assert q(b"\xc0\xaf") == '"\\xc0\\xaf"'
    assert q(b"\xed\xa0\x80") == '"\\xed\\xa0\\x80"'
    assert q(b"\xc2\x80") == '"\\u0080"'          # a valid encoding of a C1 control
    assert q(b"") == '""' and q(b"a b") == '"a b"'


FORMAT_WRITE = """name: sys_enter_write
ID: 700
format:
\tfield:unsigned short common_type;\toffset:0;\tsize:2;\tsigned:0;
\tfield:unsigned char common_flags;\toffset:2;\tsize:1;\tsigned:0;
\tfield:unsigned char common_preempt_count;\toffset:3;\tsize:1;\tsigned:0;
\tfield:int common_pid;\toffset:4;\tsize:4;\tsigned:1;

\tfield:int __syscall_nr;\toffset:8;\tsize:4;\tsigned:1;
\tfield:unsigned int fd;\toffset:16;\tsize:8;\tsigned:0;
\tfield:const char * buf;\toffset:24;\tsize:8;\tsigned:0;
\tfield:size_t count;\toffset:32;\tsize:8;\tsigned:0;

print fmt: "fd: 0x%08lx, buf: 0x%08lx, count: 0x%08lx", ((unsigned long)(REC->fd))
"""


def test_parse_syscall(G):
    d = G.parseSyscall("write", FORMAT_WRITE)
    assert d.name == "write"
    # the common_ fields stand before the empty line and are ignored; __syscall_nr (line 8) is
    # skipped; positions are line index - 8
    assert d.params == [(1, "fd"), (2, "buf"), (3, "count")]
    assert d.getParameterCount() == 3 and d.getParameterName(1) == "buf"
    with pytest.raises(IndexError):
        d.getParameterName(3)
    assert G.parseSyscall("x", "no empty line\n\tfield:int a;\toffset:0;").params == []
    assert G.parseSyscall("x", "\n field:int UPPER;\n\tfield:long long b_2;").params == [(-6, "b_2")]


def test_relate_syscall_name(G):
    pairs = {"newfstat": "fstat", "newlstat": "lstat", "newstat": "stat", "newuname": "uname",
             "sendfile64": "sendfile", "sysctl": "_sysctl", "umount": "umount2", "openat": "openat", "write": "write"}
    for k, v in pairs.items():
        assert G.relateSyscallName(k) == v


def sys_sample(mono, boot, typ, id, pid, cpu=0, comm=b"sh", args=(0,) * 6, cont_nr=0):
    raw = struct.pack("<6QQQIHH16sBB", *args, mono, boot, pid, cpu, id, comm, cont_nr, typ)
    assert len(raw) == 90
    return raw.ljust(100, b"\xaa")          # the struct's tail padding and the sample's alignment


def cont_sample(mono, index, param=b"", length=0x0FFFFFFFFFFFFFFF, failed=0):
    raw = struct.pack("<128sQQBB", param, mono, length, index, failed)
    assert len(raw) == 146
    return raw.ljust(156, b"\xbb")


def test_sample_decoder(G):
    args = (1, 2, 3, 4, 5, (1 << 64) - 1)
    samples = [sys_sample(111, 222, 1, 257, 4242, cpu=3, comm=b"cat", args=args, cont_nr=2), b"x" * 96, b"y" * 152,
               cont_sample(111, 1, b"/etc/passwd", failed=0), b"", sys_sample(5, 6, 0, 1, 2), b"z" * 157,
               cont_sample(9, 5, b"q", length=1, failed=1)]
    s, c = G.traceloop_decode(samples)
    assert len(s) == 2 and len(c) == 2 and s.dtype.itemsize == 96 and c.dtype.itemsize == 152
    r = s[0]
    assert (list(r["args"]), int(r["mono_ts"]), int(r["boot_ts"]), int(r["pid"]), int(r["cpu"]), int(r["id"]),
            r["comm"].tobytes(), int(r["cont_nr"]), int(r["typ"])) == (list(args), 111, 222, 4242, 3, 257,
                                                                      b"cat".ljust(16, b"\0"), 2, 1)
    assert int(s[1]["mono_ts"]) == 5 and int(s[1]["typ"]) == 0
    assert (c[0]["param"].tobytes().rstrip(b"\0"), int(c[0]["mono_ts"]), int(c[0]["length"]), int(c[0]["index"]),
            int(c[0]["failed"])) == (b"/etc/passwd", 111, 0x0FFFFFFFFFFFFFFF, 1, 0)
    assert (int(c[1]["mono_ts"]), int(c[1]["length"]), int(c[1]["index"]), int(c[1]["failed"])) == (9, 1, 5, 1)
    # the offsets the device decoder (igx_ingest_aos) is given
    assert dict((n, (o, w)) for n, o, w in G.TRACELOOP_SYS_FIELDS) == {
        "args": (0, 48), "mono_ts": (48, 8), "boot_ts": (56, 8), "pid": (64, 4), "cpu": (68, 2), "id": (70, 2),
        "comm": (72, 16), "cont_nr": (88, 1), "typ": (89, 1)}
    assert dict((n, (o, w)) for n, o, w in G.TRACELOOP_CONT_FIELDS) == {
        "param": (0, 128), "mono_ts": (128, 8), "length": (136, 8), "index": (144, 1), "failed": (145, 1)}
    e = G.traceloop_decode([])
    assert len(e[0]) == 0 and len(e[1]) == 0


def test_cont_param_text(G):
    p = b"ab\x01\0cd".ljust(128, b"\0")
    assert G.traceloop_cont_param(p, G.USE_NULL_BYTE_LENGTH, 0) == '"ab\\x01"'
    assert G.traceloop_cont_param(p, 1, 0) == '"a"'
    assert G.traceloop_cont_param(p, 100, 0) == '"ab\\x01"'          # FromCStringN stops at the NUL
    assert G.traceloop_cont_param(b"x" * 128, 500, 0) == '"' + "x" * 128 + '"'
    assert G.traceloop_cont_param(p, 0, 0) == '""'
    assert G.traceloop_cont_param(p, 3, 1) == '"(Failed to dereference pointer)"'


def test_events_and_extractors(G):
    s, c = G.traceloop_decode([
        sys_sample(10, 1000, 0, 1, 77, cpu=2, comm=b"cat", args=(1, 140000, 5, 9, 9, 9)),
        sys_sample(10, 1001, 1, 1, 77, args=((1 << 64) - 9, 0, 0, 0, 0, 0)),
        cont_sample(10, 1, b"hi\n", length=3),
        sys_sample(20, 2000, 0, 231, 77, comm=b"cat", args=(3, 0, 0, 0, 0, 0)),
        sys_sample(30, 3000, 1, 999, 78), sys_sample(31, 3001, 1, 0, 78, args=(7, 0, 0, 0, 0, 0))])
    names = {0: "read", 1: "write", 231: "exit_group"}
    decl = {"write": ["fd", "buf", "count"], "exit_group": G.SyscallDeclaration("exit_group", [(1, "error_code")])}
    N = 0xFFFFFFFF
    ev = G.traceloop_events(s, c, [0, 2, 3, 4], [1, N, N, N], [0, 0, 2, 2], [N, 0, N, N, N, N] + [N] * 18, names, decl,
                            mntns=4026531840, boot_to_wall_ns=5)
    assert len(ev) == 3                      # the exit of the unnamed syscall 999 is skipped
    w, x, r = ev
    assert (w.Timestamp, w.CPU, w.Pid, w.Comm, w.MountNsID, w.Syscall, w.Retval) == (1005, 2, 77, "cat", 4026531840,
                                                                                     "write", -9)
    assert [(p.Name, p.Value) for p in w.Parameters] == [("fd", "1"), ("buf", '"hi\\n"'), ("count", "5")]
    assert (x.Syscall, x.Retval, [(p.Name, p.Value) for p in x.Parameters]) == ("exit_group", 0, [("error_code", "3")])
    assert (r.Syscall, r.Retval, r.Parameters, r.Timestamp) == ("read", 7, [], 3006)
    cm = G.TraceloopColumns().cols
    assert cm["params"].Extractor(w) == 'fd=1, buf="hi\\n", count=5' and cm["ret"].Extractor(w) == "-9"
    assert cm["params"].Extractor(x) == "error_code=3" and cm["ret"].Extractor(x) == "X"
    assert cm["params"].Extractor(r) == "" and cm["ret"].Extractor(r) == "7"
    assert [k for k, col in cm.items() if not col.Visible] == ["node", "namespace", "pod", "container", "timestamp", "mntns"]
    assert (cm["cpu"].Width, cm["cpu"].FixedWidth, cm["params"].Width, cm["ret"].Width) == (3, True, 40, 3)
    # a kernel without bpf_ktime_get_boot_ns: no timestamps
    ev0 = G.traceloop_events(s, c, [0], [1], [0], [N] * 6, names, decl, have_boot_ns=False, boot_to_wall_ns=5)
    assert ev0[0].Timestamp == 0
    # an enter whose number has no name fails the read
    with pytest.raises(LookupError):
        G.traceloop_events(s, c, [3], [N], [1], [N] * 6, names, decl)
    table = G.traceloop_render(ev)
    lines = table.split("\n")
    assert lines[0].split() == ["CPU", "PID", "COMM", "SYSCALL", "PARAMS", "RET"]
    assert "write" in lines[1] and 'fd=1, buf="hi\\n", count=5' in lines[1] and lines[1].rstrip().endswith("-9")
    assert lines[2].rstrip().endswith("X")
