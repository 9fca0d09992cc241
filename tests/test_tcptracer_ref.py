"""The restatement of trace tcp (tests/tcptracer_ref.py) against hand-written cases, one per rule
of tcptracer.bpf.c, and its own consistency: the row-by-row programs with their two dicts give the
events that classify -> tuple ids -> chain join gives, for the whole stream and for the stream cut
at every position (the PASS -> HELD and the ENTER carry).  No GPU, no library."""
import numpy as np
import pytest

import tcptracer_ref as R

V4S, V4D = b"\x0a\x00\x00\x01", b"\x0a\x00\x00\x02"
V6S, V6D = bytes(range(1, 17)), bytes(range(17, 33))
SOCK = dict(family=R.AF_INET, saddr=V4S, daddr=V4D, dport=0x5000, sport=0x1F90, netns=7)


def _one(**kw):
    rows = R.make_rows([dict(SOCK, **kw)])
    return rows, R.classify_row(rows, 0)


def _key(sa, da, sport, dport, netns):
    return (sa + bytes(16 - len(sa)) + da + bytes(16 - len(da)) + sport.to_bytes(2, "little") +
            dport.to_bytes(2, "little") + netns.to_bytes(4, "little"))


def test_fill_tuple_order_and_first_zero_stops():
    rows = R.make_rows([dict(SOCK), dict(SOCK, saddr=bytes(4)), dict(SOCK, daddr=bytes(4)), dict(SOCK, dport=0),
                        dict(SOCK, sport=0), dict(SOCK, family=1)])
    assert R.fill_tuple(rows, 0, 2) == (True, _key(V4S, V4D, 0x1F90, 0x5000, 7))
    assert R.fill_tuple(rows, 1, 2) == (False, _key(b"", b"", 0, 0, 7))          # netns is read first
    assert R.fill_tuple(rows, 2, 2) == (False, _key(V4S, b"", 0, 0, 7))
    assert R.fill_tuple(rows, 3, 2) == (False, _key(V4S, V4D, 0, 0, 7))
    assert R.fill_tuple(rows, 4, 2) == (False, _key(V4S, V4D, 0, 0x5000, 7))
    assert R.fill_tuple(rows, 5, 1) == (False, _key(b"", b"", 0, 0, 7))


def test_v4_ignores_garbage_in_address_bytes_4_to_15():
    garbage = V4S + bytes(range(100, 112))
    rows = R.make_rows([dict(SOCK, saddr=garbage, daddr=V4D + b"\xff" * 12),
                        dict(SOCK, saddr=bytes(4) + b"\xff" * 12)])
    assert R.fill_tuple(rows, 0, R.AF_INET) == (True, _key(V4S, V4D, 0x1F90, 0x5000, 7))
    assert R.fill_tuple(rows, 1, R.AF_INET)[0] is False                          # only 4 bytes are tested


def test_v6_zero_test_is_over_all_16_bytes():
    rows = R.make_rows([dict(SOCK, family=10, saddr=bytes(15) + b"\x01", daddr=V6D),
                        dict(SOCK, family=10, saddr=V6S, daddr=bytes(16))])
    assert R.fill_tuple(rows, 0, R.AF_INET6) == (True, _key(bytes(15) + b"\x01", V6D, 0x1F90, 0x5000, 7))
    assert R.fill_tuple(rows, 1, R.AF_INET6) == (False, _key(V6S, b"", 0, 0, 7))


def test_filter_event_order_and_constants():
    rows = R.make_rows([dict(SOCK, pid=5, uid=6, mntns=9), dict(SOCK, family=1, pid=5, uid=6, mntns=9)])
    assert not R.filter_event(rows, 0)
    assert R.filter_event(rows, 1)                                               # family first
    assert R.filter_event(rows, 0, mntns={8}) and not R.filter_event(rows, 0, mntns={8, 9})
    assert R.filter_event(rows, 0, filter_pid=4) and not R.filter_event(rows, 0, filter_pid=5)
    assert R.filter_event(rows, 0, filter_uid=7) and not R.filter_event(rows, 0, filter_uid=6)
    assert not R.filter_event(rows, 0, filter_uid=0xFFFFFFFF)                    # (uid_t)-1: none
    rows0 = R.make_rows([dict(SOCK, uid=0)])
    assert R.filter_event(rows0, 0, filter_uid=1) and not R.filter_event(rows0, 0, filter_uid=0)


def test_connect_enter_and_return():
    assert _one(probe=R.P_ENTER)[1] == (R.ENTER, 0, bytes(40))
    assert _one(probe=R.P_ENTER, family=1)[1] == (R.NO_KIND, 0, bytes(40))
    assert _one(probe=R.P_RETURN)[1] == (R.PASS, 0, _key(V4S, V4D, 0x1F90, 0x5000, 7))
    assert _one(probe=R.P_RETURN, ret=-115)[1] == (R.ABORT, 0, bytes(40))
    assert _one(probe=R.P_RETURN, sport=0)[1] == (R.ABORT, 0, bytes(40))
    assert _one(probe=R.P_RETURN, family=1)[1] == (R.ABORT, 0, bytes(40))
    # the return probe has no filter_event
    rows = R.make_rows([dict(SOCK, probe=R.P_RETURN, pid=3)])
    assert R.classify_row(rows, 0, filter_pid=4)[0] == R.PASS


def test_set_state():
    k = _key(V4S, V4D, 0x1F90, 0x5000, 7)
    assert _one(probe=R.P_STATE, state=R.ESTABLISHED)[1] == (R.TAKE, 0, k)
    assert _one(probe=R.P_STATE, state=R.CLOSE)[1] == (R.DROP, 0, k)
    for st in (0, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12):
        assert _one(probe=R.P_STATE, state=st)[1] == (R.NO_KIND, 0, bytes(40))
    assert _one(probe=R.P_STATE, state=R.CLOSE, dport=0)[1] == (R.NO_KIND, 0, bytes(40))
    rows = R.make_rows([dict(SOCK, probe=R.P_STATE, state=R.ESTABLISHED, pid=3, uid=3, mntns=3)])
    assert R.classify_row(rows, 0, filter_pid=4, filter_uid=9, mntns={1})[0] == R.TAKE   # no filter here


def test_close():
    k = _key(V4S, V4D, 0x1F90, 0x5000, 7)
    assert _one(probe=R.P_CLOSE, state=R.ESTABLISHED)[1] == (R.NO_KIND, R.EV_CLOSE, k)
    for st in (R.SYN_SENT, R.SYN_RECV, R.NEW_SYN_RECV):
        assert _one(probe=R.P_CLOSE, state=st)[1] == (R.NO_KIND, 0, bytes(40))
    assert _one(probe=R.P_CLOSE, state=R.CLOSE, saddr=bytes(4))[1] == (R.NO_KIND, 0, bytes(40))
    rows = R.make_rows([dict(SOCK, probe=R.P_CLOSE, state=1, uid=3)])
    assert R.classify_row(rows, 0, filter_uid=4) == (R.NO_KIND, 0, bytes(40))


def test_accept_takes_sport_from_skc_num():
    # inet_sport zero, skc_num 8080: reported, with sport = bswap16(8080)
    rows, got = _one(probe=R.P_ACCEPT, sport=0, num=8080)
    assert got == (R.NO_KIND, R.EV_ACCEPT, _key(V4S, V4D, 0x901F, 0x5000, 7))
    assert _one(probe=R.P_ACCEPT, sport=0x1F90, num=0)[1] == (R.NO_KIND, 0, bytes(40))
    # fill_tuple stopped at saddr, so daddr and dport are still zero: dropped
    assert _one(probe=R.P_ACCEPT, saddr=bytes(4), num=80)[1] == (R.NO_KIND, 0, bytes(40))
    assert _one(probe=R.P_ACCEPT, dport=0, num=80)[1] == (R.NO_KIND, 0, bytes(40))
    assert _one(probe=R.P_ACCEPT, family=10, saddr=V6S, daddr=V6D, num=80)[1][1] == R.EV_ACCEPT


def test_chain_join_hand_cases():
    E, P, A, T, D, H = R.ENTER, R.PASS, R.ABORT, R.TAKE, R.DROP, R.HELD
    x = [1] * 8

    def cj(kinds, k1=None, k2=None):
        return R.chain_join(k1 or x[:len(kinds)], k2 or x[:len(kinds)], kinds)

    assert cj([E, P, T]) == ([(2, 1)], [])
    assert cj([P, T]) == ([], [])                       # PASS without ENTER
    assert cj([T]) == ([], [])                          # TAKE without PASS
    assert cj([E, A, T]) == ([], [])
    assert cj([E, P, D, T]) == ([], [])                 # DROP then TAKE
    assert cj([E, P, T, T]) == ([(2, 1)], [])
    assert cj([H, T]) == ([(1, 0)], [])
    assert cj([E, P, E, P, T]) == ([(4, 3)], [])        # a second PASS overwrites the first
    assert cj([E, E, P]) == ([], [2])
    assert cj([E, P, E]) == ([], [1, 2])
    assert cj([E, E, P, T], k1=[1, 2, 1, 9], k2=[5, 5, 5, 5]) == ([(3, 2)], [1])
    assert R.chain_join(x[:3], x[:3], [E, P, T], valid=[1, 0, 1]) == ([], [0])


def _stream(seed, n=90):
    """A probe stream over few threads and sockets so that the maps are hit from every side."""
    rng = np.random.default_rng(seed)
    socks = [dict(family=2, saddr=V4S, daddr=V4D, dport=0x5000, sport=0x100 + s, netns=1) for s in range(3)]
    socks += [dict(family=10, saddr=V6S, daddr=V6D, dport=0x5000, sport=0x200, netns=1),
              dict(family=2, saddr=V4S, daddr=V4D, dport=0x5000, sport=0, num=80, netns=1)]
    specs = []
    for _ in range(n):
        probe = int(rng.choice(5, p=[0.25, 0.25, 0.1, 0.3, 0.1]))
        s = dict(socks[int(rng.integers(0, len(socks)))], probe=probe, tid=int(rng.integers(1, 4)),
                 pid=int(rng.integers(1, 3)), uid=int(rng.integers(0, 2)), mntns=int(rng.integers(1, 3)))
        if probe == R.P_RETURN:
            s["ret"] = int(rng.choice([0, 0, 0, -111]))
        if probe in (R.P_STATE, R.P_CLOSE):
            s["state"] = int(rng.choice([1, 1, 1, 7, 2]))
        specs.append(s)
    return R.make_rows(specs)


@pytest.mark.parametrize("flt", [{}, {"filter_pid": 1}, {"filter_uid": 1}, {"mntns": [2]}])
def test_every_cut_gives_the_whole_stream(flt):
    total = 0
    for seed in (1, 2, 3):
        rows = _stream(seed)
        whole = R.trace(rows, **flt)
        assert R.trace_via_join(rows, **flt) == whole
        for cut in range(1, len(rows["probe"])):
            assert R.trace_via_join(rows, cuts=(cut,), **flt) == whole, cut
        total += sum(1 for e in whole if e[0] == "connect")
    assert total >= 5
    # and both carries occur at some cut: an ENTER and a PASS pending
    rows = _stream(1)
    c = R.classify(rows, **flt)
    key2 = np.array([hash(bytes(t)) & 0xFFFFFFFF for t in c["tuple"]], np.uint64)
    carried = set()
    for cut in range(1, len(rows["probe"])):
        _, live = R.chain_join(c["key1"][:cut], key2[:cut], c["kind"][:cut])
        carried |= {int(c["kind"][i]) for i in live}
    assert carried == {R.ENTER, R.PASS}
