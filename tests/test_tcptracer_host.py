"""trace tcp's host side (gadgets.py) without a GPU: the event built from a probe's tuple, the
columns and their tags, the JSON names, the `t` extractor and the render, against expectations
written by hand from pkg/gadgets/trace/tcp/types/types.go and tracer/tracer.go:198-228.  This is
not a Go run: nothing here was produced by the reference's own code."""
import json

import tcptracer_ref as R


def _tuple(sa, da, sport_net, dport_net, netns=7):
    return (sa + bytes(16 - len(sa)) + da + bytes(16 - len(da)) + sport_net.to_bytes(2, "big") +
            dport_net.to_bytes(2, "big") + netns.to_bytes(4, "little"))


def _ev(G, op=3, fam=2, sa=b"\x0a\x00\x00\x01", da=b"\xc0\xa8\x01\x02", sport=43210, dport=443, **kw):
    args = dict(pid=77, mntns=4026531840, comm=b"curl\0junk", ts=5000, boot_to_wall_ns=7)
    args.update(kw)
    return G.tcp_event(op, fam, _tuple(sa, da, sport, dport), **args)


def test_htons(igx):
    G = igx.gadgets
    assert G.Htons(0x1F90) == 0x901F and G.Htons(0x0050) == 0x5000 and G.Htons(0) == 0 and G.Htons(0xFFFF) == 0xFFFF
    assert G.Htons(G.Htons(8080)) == 8080


def test_event_fields(igx):
    G = igx.gadgets
    e = _ev(G)
    assert (e.Operation, e.Pid, e.Comm, e.IPVersion, e.Saddr, e.Daddr, e.Sport, e.Dport) == \
        ("connect", 77, "curl", 4, "10.0.0.1", "192.168.1.2", 43210, 443)
    assert (e.Timestamp, e.MountNsID, e.Type) == (5007, 4026531840, "normal")
    assert _ev(G, op=1).Operation == "accept" and _ev(G, op=2).Operation == "close" and _ev(G, op=9).Operation == ""
    v6 = _ev(G, fam=10, sa=bytes.fromhex("20010db8000000000000000000000001"), da=bytes(15) + b"\x01")
    assert (v6.IPVersion, v6.Saddr, v6.Daddr) == (6, "2001:db8::1", "::1")
    mapped = _ev(G, fam=10, sa=bytes(10) + b"\xff\xff\x0a\x00\x00\x01")
    assert mapped.Saddr == "::ffff:10.0.0.1"
    other = _ev(G, fam=1)
    assert (other.IPVersion, other.Saddr, other.Daddr) == (0, "", "")


def test_columns_and_extractor(igx):
    G = igx.gadgets
    cm = G.TraceTcpColumns().cols
    assert list(cm) == ["node", "namespace", "pod", "container", "timestamp", "mntns", "t", "pid", "comm", "ip", "saddr",
                        "daddr", "sport", "dport"]
    assert [k for k, c in cm.items() if not c.Visible] == ["node", "namespace", "pod", "container", "timestamp", "mntns"]
    assert (cm["t"].Width, cm["t"].FixedWidth, cm["ip"].Width, cm["ip"].FixedWidth) == (1, True, 2, True)
    assert cm["node"].Tags == ["kubernetes"] and cm["container"].Tags == ["kubernetes", "runtime"]
    t = cm["t"].Extractor
    assert [t(_ev(G, op=o)) for o in (1, 3, 2, 9)] == ["A", "C", "X", "U"]
    e = _ev(G)
    e.Operation = "unknown"
    assert t(e) == "U"


def test_render(igx):
    G = igx.gadgets
    evs = [_ev(G), _ev(G, op=1, sport=80, dport=51000, comm=b"nginx"), _ev(G, op=2, fam=10, sa=bytes(15) + b"\x01",
                                                                         da=bytes(15) + b"\x02")]
    lines = G.tcp_render(evs).split("\n")
    assert lines[0].split() == ["T", "PID", "COMM", "IP", "SADDR", "DADDR", "SPORT", "DPORT"]
    assert lines[1].split() == ["C", "77", "curl", "4", "10.0.0.1", "192.168.1.2", "43210", "443"]
    assert lines[2].split() == ["A", "77", "nginx", "4", "10.0.0.1", "192.168.1.2", "80", "51000"]
    assert lines[3].split() == ["X", "77", "curl", "6", "::1", "::2", "43210", "443"]
    shown = G.tcp_render(evs[:1], columns=["t", "mntns", "dport"]).split("\n")
    assert shown[0].split() == ["T", "MNTNS", "DPORT"] and shown[1].split() == ["C", "4026531840", "443"]


def test_json_names_and_omitempty(igx):
    G = igx.gadgets
    d = json.loads(G.tcp_event_json(_ev(G)))
    assert d == {"timestamp": 5007, "type": "normal", "mountnsid": 4026531840, "operation": "connect", "pid": 77,
                 "comm": "curl", "ipversion": 4, "saddr": "10.0.0.1", "daddr": "192.168.1.2", "sport": 43210,
                 "dport": 443}
    assert list(d) == ["timestamp", "type", "mountnsid", "operation", "pid", "comm", "ipversion", "saddr", "daddr",
                       "sport", "dport"]
    e = G.TcpEvent(Node="n1", Pod="p")
    assert json.loads(G.tcp_event_json(e)) == {"node": "n1", "pod": "p", "type": "normal"}     # omitempty; type stays


def test_restatement_to_event(igx):
    """tests/tcptracer_ref.py's to_event, which the device tests compare with, against tcp_event."""
    G = igx.gadgets
    sock = dict(family=2, saddr=b"\x0a\x00\x00\x01", daddr=b"\x0a\x00\x00\x02", dport=0xBB01, sport=0x1F90, netns=7)
    rows = R.make_rows([dict(sock, probe=R.P_ENTER, tid=5, pid=4, mntns=9, comm=b"a"),
                        dict(sock, probe=R.P_RETURN, tid=5, pid=4, mntns=9, comm=b"curl"),
                        dict(sock, probe=R.P_STATE, state=1, tid=99, pid=98, mntns=1, comm=b"swapper"),
                        dict(sock, probe=R.P_ACCEPT, sport=0, num=8080, pid=3, comm=b"srv")])
    out = R.trace(rows)
    assert out == [("connect", 2, 1), ("accept", 3, 3)]
    d = R.to_event(rows, out[0], 3)
    assert d == {"Operation": "connect", "Timestamp": 3003, "MountNsID": 9, "Pid": 4, "Comm": "curl", "IPVersion": 4,
                 "Saddr": "10.0.0.1", "Daddr": "10.0.0.2", "Sport": 0x901F, "Dport": 0x01BB}
    e = G.tcp_event(3, 2, R.classify_row(rows, 2)[2], 4, 9, b"curl" + bytes(12), 3000, 3)
    assert d == {k: getattr(e, k) for k in d}
    assert R.to_event(rows, out[1])["Sport"] == 8080
