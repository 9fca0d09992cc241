"""gadgets.TraceTcpTracer end to end on the device, a few hundred rows at most, against the
row-by-row restatement of the BPF programs in tests/tcptracer_ref.py (trace + to_event): every
field of every event, in order.  Filtered-at-entry connects stay silent although their
tcp_set_state rows arrive; a connect's task comes from the return row; accept / close / connect
interleave in row order; batch boundaries between enter and return and between return and
established; a pending overflow raises."""
import numpy as np
import pytest

import tcptracer_ref as R

pytestmark = pytest.mark.gpu

A, B = b"\x0a\x00\x00\x01", b"\x0a\x00\x00\x02"
FIELDS = ("Operation", "Timestamp", "MountNsID", "Pid", "Comm", "IPVersion", "Saddr", "Daddr", "Sport", "Dport")


def sock(i, v6=False):
    if v6:
        return dict(family=10, saddr=bytes(15) + bytes([1 + i % 200]), daddr=bytes(range(1, 17)), dport=0xBB01,
                    sport=0x1000 + i, netns=4026531992)
    return dict(family=2, saddr=A, daddr=B, dport=0x5000, sport=0x1000 + i, netns=4026531992)


def task(i):
    return dict(tid=1000 + i, pid=500 + i // 2, uid=i % 3, mntns=4026532000 + i % 4, comm=b"task%d" % i)


def kernel():
    """The context tcp_set_state usually runs in: some other task."""
    return dict(tid=7, pid=7, uid=0, mntns=4026531840, comm=b"ksoftirqd/3")


def connect(i, s=None, ret=0, v6=False):
    s = sock(i, v6) if s is None else s
    fam = dict(family=s["family"])
    return [dict(s, probe=R.P_ENTER, **task(i)), dict(s, probe=R.P_RETURN, ret=ret, **dict(task(i), **fam)),
            dict(s, probe=R.P_STATE, state=R.ESTABLISHED, **kernel())]


def _feed(igx, tracer, rows, cuts=()):
    H = igx.columns
    out, pending = [], []
    bounds = [0] + list(cuts) + [len(rows["probe"])]
    for a, b in zip(bounds[:-1], bounds[1:]):
        out += tracer.feed({k: H.to_device(np.ascontiguousarray(rows[k][a:b])) for k in igx.gadgets.TCP_TRACE_COLS})
        pending.append(tracer.pending)
    return [{k: getattr(e, k) for k in FIELDS} for e in out], pending


def _want(rows, boot=0, **flt):
    ev = R.trace(rows, **flt)
    return ev, [R.to_event(rows, e, boot) for e in ev]


def test_filtered_at_entry_connects_stay_silent(igx):
    specs = []
    for i in range(12):
        specs += connect(i, v6=i % 5 == 0)
    rows = R.make_rows(specs)
    G = igx.gadgets
    for flt, kw in (({}, {}), ({"filter_pid": 502}, {"filter_pid": 502}), ({"filter_uid": 1}, {"filter_uid": 1}),
                    ({"mntns": [4026532001, 4026532003]}, {"mntns_filter": [4026532003, 4026532001]}),
                    ({"filter_pid": 503, "filter_uid": 0, "mntns": [4026532002]},
                     {"filter_pid": 503, "filter_uid": 0, "mntns_filter": [4026532002]})):
        ev, want = _want(rows, **flt)
        # every tcp_set_state row arrives whatever the filter; only admitted connects speak
        assert 0 < len(ev) < 12 if flt else len(ev) == 12
        got, _ = _feed(igx, G.TraceTcpTracer(**kw), rows)
        assert got == want, flt


def test_connect_task_comes_from_the_return_row(igx):
    rows = R.make_rows(connect(3) + connect(4, v6=True))
    ev, want = _want(rows, boot=11)
    assert ev == [("connect", 2, 1), ("connect", 5, 4)]
    got, _ = _feed(igx, igx.gadgets.TraceTcpTracer(boot_to_wall_ns=11), rows)
    assert got == want
    assert [(g["Pid"], g["Comm"], g["MountNsID"]) for g in got] == [(501, "task3", 4026532003), (502, "task4", 4026532000)]
    assert got[0]["Timestamp"] == int(rows["ts"][2]) + 11        # the established row's time, not the return's


def test_events_interleave_in_row_order(igx):
    c0, c1 = connect(0), connect(1, v6=True)
    acc = dict(sock(50), probe=R.P_ACCEPT, sport=0, num=8080, **task(9))          # inet_sport 0, skc_num set
    acc_zero = dict(sock(51), probe=R.P_ACCEPT, num=0, **task(9))
    clo = dict(sock(0), probe=R.P_CLOSE, state=R.ESTABLISHED, **task(0))
    clo_syn = dict(sock(52), probe=R.P_CLOSE, state=R.SYN_SENT, **task(2))
    garbage = dict(sock(53), probe=R.P_CLOSE, state=R.CLOSE, **task(2))
    garbage["saddr"] = A + bytes(range(100, 112))                                # v4: bytes 4..15 are not read
    drop = dict(sock(1, True), probe=R.P_STATE, state=R.CLOSE, **kernel())
    specs = [c0[0], acc, c1[0], c0[1], clo_syn, c1[1], acc_zero, c0[2], garbage, clo, drop, c1[2], acc]
    rows = R.make_rows(specs)
    ev, want = _want(rows)
    assert [(t, r) for t, r, _ in ev] == [("accept", 1), ("connect", 7), ("close", 8), ("close", 9), ("accept", 12)]
    got, _ = _feed(igx, igx.gadgets.TraceTcpTracer(), rows)
    assert got == want
    assert got[0]["Sport"] == 8080 and got[2]["Saddr"] == "10.0.0.1"


@pytest.mark.parametrize("cut,carried", [(1, "enter"), (2, "held")])
def test_batch_boundary_inside_a_connect(igx, cut, carried):
    """cut 1 falls between enter and return (the ENTER row is carried), cut 2 between return and
    established (the admitted PASS is carried as HELD).  Other connections surround it."""
    pre, me, post = connect(0), connect(1), connect(2)
    specs = pre[:2] + me[:cut] + [post[0]]
    n_first = len(specs)
    specs += me[cut:] + [pre[2]] + post[1:]
    rows = R.make_rows(specs)
    ev, want = _want(rows)
    assert len(ev) == 3
    tr = igx.gadgets.TraceTcpTracer()
    got, pending = _feed(igx, tr, rows, cuts=(n_first,))
    assert got == want
    assert pending == [3, 0]              # pre's HELD, mine (ENTER or HELD), post's ENTER; then nothing
    kinds = sorted(int(k) for k in igx.columns.host(_carry_kinds(igx, rows, n_first)))
    assert kinds == ([R.ENTER, R.ENTER, R.HELD] if carried == "enter" else [R.ENTER, R.HELD, R.HELD])


def _carry_kinds(igx, rows, n_first):
    H = igx.columns
    tr = igx.gadgets.TraceTcpTracer()
    tr.feed({k: H.to_device(np.ascontiguousarray(rows[k][:n_first])) for k in igx.gadgets.TCP_TRACE_COLS})
    return tr._carry["_kind"]


def _overlapping_stream(rng):
    """40 connections over 16 tasks and 6 sockets, eight open at a time with their rows interleaved,
    some failing, with close / accept / set-state rows of other tasks between them."""
    open_, specs = [], []
    for i in range(40):
        open_.append(connect(i % 16, sock(i % 6, v6=i % 4 == 0), ret=0 if rng.random() > 0.15 else -111))
    heads = [0] * len(open_)
    live = list(range(8))
    nxt = 8
    while live:
        j = int(rng.integers(0, len(live)))
        c = live[j]
        specs.append(open_[c][heads[c]])
        heads[c] += 1
        if heads[c] == 3:
            live.pop(j)
            if nxt < len(open_):
                live.append(nxt)
                nxt += 1
        if rng.random() < 0.2:
            specs.append(dict(sock(int(rng.integers(0, 6))), probe=int(rng.choice([R.P_CLOSE, R.P_ACCEPT, R.P_STATE])),
                              state=int(rng.choice([1, 7, 2])), num=int(rng.choice([0, 80])), **task(int(rng.integers(0, 16)))))
    return specs


def test_carried_rows_meet_no_filter_again_and_every_cut_agrees(igx):
    """A stream of a few hundred rows, unfiltered and under a pid and a mount-namespace filter, cut
    at 5 places: the events of the whole stream."""
    rng = np.random.default_rng(5)
    specs = _overlapping_stream(rng)
    rows = R.make_rows(specs)
    n = len(specs)
    assert 120 < n < 400
    for flt, kw in (({}, {}), ({"filter_pid": 503}, {"filter_pid": 503}), ({"mntns": [4026532001]}, {"mntns_filter": [4026532001]})):
        ev, want = _want(rows, **flt)
        assert sum(1 for e in ev if e[0] == "connect") >= 3
        cuts = sorted(int(x) for x in rng.choice(np.arange(1, n), 5, replace=False))
        got, pending = _feed(igx, igx.gadgets.TraceTcpTracer(**kw), rows, cuts)
        assert got == want, (flt, cuts)
        assert flt or min(pending[:-1]) > 0          # eight connections are open at any cut
        got1, _ = _feed(igx, igx.gadgets.TraceTcpTracer(**kw), rows)
        assert got1 == want


def test_pending_overflow_raises(igx):
    specs = []
    for i in range(9):
        specs += connect(i)[:1 + i % 2]          # enters, some with their return: ENTER and PASS rows stay
    rows = R.make_rows(specs)
    tr = igx.gadgets.TraceTcpTracer(pending_cap=8)
    with pytest.raises(igx._abi.IgxError) as e:
        _feed(igx, tr, rows)
    assert e.value.code == igx._abi.IGX_ENOSPC and "9 map entries" in str(e.value)
    ok = igx.gadgets.TraceTcpTracer(pending_cap=9)
    assert _feed(igx, ok, rows) == ([], [9])
