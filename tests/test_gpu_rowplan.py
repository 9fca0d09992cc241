"""Row plans of the cached group-by (k_gb_table.h RowPlan; DESIGN.md §4 "Row plans").

A cached update whose shape is exactly what gadgets.TopTcpTracer / TopFileTracer build runs a
kernel instance compiled for that shape (igx_groupby_rowplan reports 1 / 2); every other shape,
and every update under IGX_GB_ROWPLAN=0, runs the general kernel (0).  Both must give the
oracle's table bit for bit: every group's key, sums and first index, and the group count.

Every case runs twice, specialised and with IGX_GB_ROWPLAN=0, in IGX_GB_CACHED, against
oracle.groupby (or_groupby) over the same rows with the probe's drops as its valid mask; the
top-tcp cases also against oracle.top_tcp (or_top_tcp), which applies tcptop's checks itself.

Row counts 1, 63, 64, 65, 4097, 70001: the tail lanes of a wave, more than one loader step and
more than one workgroup, and the 1-byte (dir, op) and 2-byte (family, ports) columns read at
their own width at every row & 3.  Planted rows (same on both sides):
  top tcp   family outside {2, 10}; size >= 2^31 on receives (`int copied` <= 0: dropped) and on
            sends (kept); size 0 (a receive is dropped, a send counts 0); rows 128..255 all dropped
  top file  op 0, 1 and 2 (neither READ nor WRITE: the group exists, nothing is added);
            count 0 and 2^32 - 1
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 4097, 70001)
NMAX = max(NS)
GK = 3000                       # distinct keys: more than the rows of the small cases, fewer than the large one's
TCP_NAMES = ("saddr", "daddr", "mntns", "pid", "comm", "lport", "dport", "family", "size", "dir")
TCP_KEY = TCP_NAMES[:8]
FILE_NAMES = ("inode", "dev", "pid", "tid", "op", "count")
FILE_KEY = FILE_NAMES[:4]


@pytest.fixture(scope="module")
def E(igx):
    return igx.engine


@pytest.fixture(scope="module")
def H(igx):
    return igx.columns


@pytest.fixture(scope="module")
def A(igx):
    return igx._abi


def _family_in(A, col, negate=0):
    p = A.Pred()
    p.col, p.cmp, p.negate, p.ref_len = col, A.CMP_IN, negate, 4
    for i, b in enumerate((2).to_bytes(2, "little") + (10).to_bytes(2, "little")):
        p.ref[i] = b
    return p


def _copied(A, col, dir_col):
    p = A.Pred()
    p.col, p.cmp, p.negate, p.ref_len = col, A.CMP_GT, 0, 4
    p.guard_col, p.guard_len, p.guard_ref[0] = dir_col, 1, 1
    return p


@pytest.fixture(scope="module")
def tcp(oracle, H, torch):
    """NMAX top-tcp rows with the planted ones, on the host and on the device (a smaller case reads
    a prefix), and what the probe keeps of them."""
    O = oracle
    ev = O.gen_tcp(0x70, 0, GK, O.zipf_cdf(GK, 1.1), 0, NMAX)
    ev["family"][6::7] = 3
    ev["size"][3::11] |= np.uint32(0x80000000)
    ev["size"][5::13] = 0
    ev["family"][128:256] = 7
    ev["dir"][0] = 0            # the one-row case keeps its row
    assert {0, 1} <= set(ev["dir"][:63].tolist()), "both probes within the smallest multi-row case"
    keep = np.isin(ev["family"], (2, 10)) & ~((ev["dir"] == 1) & (ev["size"].view(np.int32) <= 0))
    assert keep[0] and not keep[128:256].any()
    big = ev["size"] >= 1 << 31
    assert (big & (ev["dir"] == 0) & keep)[:4097].any() and (big & (ev["dir"] == 1))[:4097].any()
    dev = {k: H.to_device(v) for k, v in ev.items()}
    return {"h": ev, "d": dev, "keep": keep, "keys": O.pad_keys(ev, TCP_KEY)}


@pytest.fixture(scope="module")
def filev(oracle, H):
    O = oracle
    ev = O.gen_file(0x75, 0, GK, O.zipf_cdf(GK, 1.05), 0, NMAX)
    ev["op"][::5] = 2
    ev["count"][1::7] = 0
    ev["count"][2::9] = 0xFFFFFFFF
    assert {0, 1, 2} <= set(ev["op"][:63].tolist())
    dev = {k: H.to_device(v) for k, v in ev.items()}
    return {"h": ev, "d": dev, "keys": O.pad_keys(ev, FILE_KEY)}


@pytest.fixture(scope="module")
def tcp_tab(E, A):
    t = E.Table([16, 16, 8, 4, 16, 2, 2, 2], [A.Agg(A.AGG_SUM, 8, 9, 8, 0), A.Agg(A.AGG_SUM, 8, 9, 8, 1)], 2 * GK)
    t.set_mode(A.GB_CACHED)
    yield t
    t.destroy()


@pytest.fixture(scope="module")
def file_tab(E, A):
    aggs = [A.Agg(A.AGG_COUNT, 0, 4, 8, 0), A.Agg(A.AGG_SUM, 5, 4, 8, 0),
            A.Agg(A.AGG_COUNT, 0, 4, 8, 1), A.Agg(A.AGG_SUM, 5, 4, 8, 1)]
    t = E.Table([8, 4, 4, 4], aggs, 2 * GK)
    t.set_mode(A.GB_CACHED)
    yield t
    t.destroy()


def _table(E, H, tab):
    """{key bytes: (aggregates..., first index)} of the finalized table, and its group count."""
    fin = tab.finalize()
    keys, aggs, first = E.table_tensors(tab, fin)
    hk, ha, hf = H.host(keys), [H.host(a) for a in aggs], H.host(first)
    got = {hk[i].tobytes(): tuple(int(a[i]) for a in ha) + (int(hf[i]),) for i in range(len(hk))}
    assert len(got) == len(hk), "duplicate groups"
    return got, fin["n_groups"]


def _want(oracle, keys, aggs, keep, base):
    ok, oa, of = oracle.groupby(keys, aggs, valid=keep, base_idx=base)
    return {ok[i].tobytes(): tuple(int(a[i]) for a in oa[:len(aggs)]) + (int(of[i]),) for i in range(len(ok))}


def _tcp_aggs(h, n, val="size"):
    return [{"kind": "sum", "val": h[val][:n], "cond": h["dir"][:n], "cond_val": 0},
            {"kind": "sum", "val": h[val][:n], "cond": h["dir"][:n], "cond_val": 1}]


def _file_aggs(h, n):
    return [{"kind": "count", "cond": h["op"][:n], "cond_val": 0},
            {"kind": "sum", "val": h["count"][:n], "cond": h["op"][:n], "cond_val": 0},
            {"kind": "count", "cond": h["op"][:n], "cond_val": 1},
            {"kind": "sum", "val": h["count"][:n], "cond": h["op"][:n], "cond_val": 1}]


def _both_ways(monkeypatch, run, plan):
    """run() once specialised (it must report `plan`) and once under IGX_GB_ROWPLAN=0 (0)."""
    monkeypatch.delenv("IGX_GB_ROWPLAN", raising=False)
    assert run() == plan
    monkeypatch.setenv("IGX_GB_ROWPLAN", "0")
    assert run() == 0


@pytest.mark.parametrize("n,base", [(n, 0) for n in NS] + [(65, (1 << 33) + 5)])
def test_top_tcp_plan(E, H, A, oracle, torch, monkeypatch, tcp, tcp_tab, n, base):
    h, d = tcp["h"], tcp["d"]
    cols = [d[k][:n] for k in TCP_NAMES] + [d["size"][:n].view(torch.int32)]
    want = _want(oracle, tcp["keys"][:n], _tcp_aggs(h, n), tcp["keep"][:n], base)
    # or_top_tcp applies the probe's own drops: the same groups, every one of them (k = all)
    G, tk, ts, tr, tf = oracle.top_tcp({k: v[:n] for k, v in h.items()}, k=max(1, len(want)), base_idx=base, max_groups=n)
    assert G == len(want)
    pk = np.zeros((G, 72), np.uint8)    # ip_key_t packs its three u16 fields; the table pads each to 4 bytes
    pk[:, :60] = tk[:, :60]
    for j in range(3):
        pk[:, 60 + 4 * j:62 + 4 * j] = tk[:, 60 + 2 * j:62 + 2 * j]
    assert {pk[i].tobytes(): (int(ts[i]), int(tr[i]), int(tf[i])) for i in range(G)} == want

    def run():
        tcp_tab.reset()
        tcp_tab.update(cols, list(range(8)), n, base, [_family_in(A, 7), _copied(A, 10, 9)])
        plan = tcp_tab.rowplan()
        got, ng = _table(E, H, tcp_tab)
        assert ng == len(want) and got == want
        return plan

    _both_ways(monkeypatch, run, 1)


@pytest.mark.parametrize("n", NS)
def test_top_file_plan(E, H, A, oracle, monkeypatch, filev, file_tab, n):
    h, d = filev["h"], filev["d"]
    cols = [d[k][:n] for k in FILE_NAMES]
    want = _want(oracle, filev["keys"][:n], _file_aggs(h, n), None, 0)

    def run():
        file_tab.reset()
        file_tab.update(cols, [0, 1, 2, 3], n, 0)
        plan = file_tab.rowplan()
        got, ng = _table(E, H, file_tab)
        assert ng == len(want) and got == want
        return plan

    _both_ways(monkeypatch, run, 2)


@pytest.mark.parametrize("near", ["negated-family", "valid-column", "8-byte-value", "index-column"])
def test_near_miss_plans_run_general(E, H, A, oracle, torch, monkeypatch, tcp, near):
    """The top-tcp shape with one field changed is no registered plan: the general kernel runs it."""
    n = 4097
    h, d = tcp["h"], tcp["d"]
    monkeypatch.delenv("IGX_GB_ROWPLAN", raising=False)
    cols = [d[k][:n] for k in TCP_NAMES] + [d["size"][:n].view(torch.int32)]
    preds = [_family_in(A, 7), _copied(A, 10, 9)]
    keep, aggs, kw = tcp["keep"][:n], _tcp_aggs(h, n), {}
    if near == "negated-family":
        preds[0] = _family_in(A, 7, negate=1)
        keep = ~np.isin(h["family"][:n], (2, 10)) & ~((h["dir"][:n] == 1) & (h["size"][:n].view(np.int32) <= 0))
        assert keep.any()
    elif near == "valid-column":
        valid = (np.arange(n) % 3 != 1).astype(np.uint8)
        kw["valid"] = H.to_device(valid)
        keep = keep & (valid != 0)
    elif near == "8-byte-value":
        size64 = h["size"][:n].astype(np.uint64) << np.uint64(3)
        cols[8] = H.to_device(size64)
        cols[10] = d["size"][:n].clone().view(torch.int32)   # `copied` stays the 4-byte column
        aggs = _tcp_aggs({"size": size64, "dir": h["dir"]}, n)
    else:
        cols.append(torch.arange(n, dtype=torch.int64, device=cols[0].device).view(torch.uint64))
        kw["idx_col"] = 11
    want = _want(oracle, tcp["keys"][:n], aggs, keep, 0)
    tab = E.Table([16, 16, 8, 4, 16, 2, 2, 2], [A.Agg(A.AGG_SUM, 8, 9, 8, 0), A.Agg(A.AGG_SUM, 8, 9, 8, 1)], 2 * GK)
    try:
        tab.set_mode(A.GB_CACHED)
        tab.update(cols, list(range(8)), n, 0, preds, **kw)
        assert tab.rowplan() == 0
        got, ng = _table(E, H, tab)
        assert ng == len(want) and got == want
    finally:
        tab.destroy()


def test_two_updates_one_interval(E, H, A, oracle, torch, monkeypatch, tcp, tcp_tab):
    """An interval fed by a specialised update and then a general one is one table."""
    n, cut = 4097, 2048
    h, d = tcp["h"], tcp["d"]
    preds = [_family_in(A, 7), _copied(A, 10, 9)]
    want = _want(oracle, tcp["keys"][:n], _tcp_aggs(h, n), tcp["keep"][:n], 0)
    tcp_tab.reset()
    for a, b, env, plan in ((0, cut, None, 1), (cut, n, "0", 0)):
        if env is None:
            monkeypatch.delenv("IGX_GB_ROWPLAN", raising=False)
        else:
            monkeypatch.setenv("IGX_GB_ROWPLAN", env)
        cols = [d[k][a:b] for k in TCP_NAMES] + [d["size"][a:b].view(torch.int32)]
        tcp_tab.update(cols, list(range(8)), b - a, a, preds)
        assert tcp_tab.rowplan() == plan
    got, ng = _table(E, H, tcp_tab)
    assert ng == len(want) and got == want
