"""igx_traceloop_join (traceloop's enter / exit / cont join on the device) against the row-by-row
restatement of Tracer.Read in tests/traceloop_ref.py: every output array and the count, exactly.

Sizes: the hand-worked groups of tests/test_traceloop_ref.py, alone and in one call; ns in
{0, 1, T-1, T, T+1, 2T+1} with no conts and with about ns/2 (T is the scan tile, from the
library); one group of 3T rows; groups whose rows lie tiles apart in the sorted order and in
the stream; random streams of about 50 000 rows with a tenth of the timestamps colliding, valid
masks on both streams, one and 300 containers, both sort timestamps and both sync modes; two calls
on one input; the argument errors on a live context."""
import ctypes as C

import numpy as np
import pytest

import traceloop_ref as R
from test_traceloop_ref import CASES, columns

pytestmark = pytest.mark.gpu

DT = dict(mono_ts=np.uint64, sort_ts=np.uint64, typ=np.uint8, id=np.uint16, pid=np.uint32, valid=np.uint8,
          mntns=np.uint64, c_mono_ts=np.uint64, c_index=np.uint8, c_valid=np.uint8, c_mntns=np.uint64)


def as_arrays(col):
    return {k: np.asarray(v, dtype=DT[k]) for k, v in col.items() if v is not None}


def device_join(igx, col, sync=True, nr=R.NR_X86_64):
    H = igx.columns
    d = {k: H.to_device(v) for k, v in as_arrays(col).items()}
    j = igx.engine.traceloop_join(d["mono_ts"], d["sort_ts"], d["typ"], d["id"], d["pid"], valid=d.get("valid"),
                                  mntns=d.get("mntns"), c_mono_ts=d.get("c_mono_ts"), c_index=d.get("c_index"),
                                  c_valid=d.get("c_valid"), c_mntns=d.get("c_mntns"), nr=nr, sync=sync)
    nev = j["n_events"] if sync else int(H.host(j["n_events"])[0])
    full = {k: H.host(j[k]) for k in ("row", "exit", "cls", "cont")}
    got = (full["row"][:nev].view(np.uint32), full["exit"][:nev].view(np.uint32), full["cls"][:nev],
           full["cont"][:nev].reshape(-1).view(np.uint32))
    return got, nev, full


def check(igx, col, sync=True, nr=R.NR_X86_64):
    want = R.join(**col, nr=nr)
    got, nev, full = device_join(igx, col, sync, nr)
    assert nev == len(want[0])
    for g, w, name in zip(got, want, ("row", "exit", "class", "cont")):
        assert np.array_equal(g, np.asarray(w, dtype=g.dtype)), name
    return want, full


@pytest.mark.parametrize("case", CASES, ids=[c[0].split()[0] for c in CASES])
def test_hand_worked_group(igx, case):
    _, rows, crows, expect = case
    want, _ = check(igx, columns(rows, crows))
    assert [(want[0][j], want[1][j], want[2][j], want[3][6 * j:6 * j + 6]) for j in range(len(expect))] == expect


def test_hand_worked_groups_in_one_call(igx):
    rows, crows = [], []
    for k, (_, r, c, _) in enumerate(CASES):
        base = 1000 * (k + 1)
        rows += [(base + x[0],) + tuple(x[1:4]) + (base + (x[4] if len(x) > 4 else x[0]),) + tuple(x[5:6] or (1,)) for x in r]
        crows += [(base + x[0], x[1]) + tuple(x[2:3] or (1,)) for x in c]
    want, _ = check(igx, columns(rows, crows))
    assert len(want[0]) == sum(len(c[3]) for c in CASES)


def stream(ns, nc, seed, containers=1, collide=0.1, masks=False, sort="boot"):
    """A seeded stream of ns syscall rows and nc cont rows: syscalls as enter / exit pairs on a
    timestamp of their own (some enters or exits lost, some of exit_group), a share `collide` of
    the timestamps drawn from a small pool so that groups hold several syscalls, conts on the
    timestamps of random rows."""
    rng = np.random.default_rng(seed)
    npair = ns // 2 + 1
    ts = rng.permutation(npair).astype(np.uint64) * np.uint64(1000) + np.uint64(10**12)
    hit = rng.random(npair) < collide
    ts[hit] = np.uint64(10**12 + 7) + rng.integers(0, max(1, npair // 100), int(hit.sum())).astype(np.uint64) * np.uint64(1000)
    pid = rng.integers(1, 40, npair).astype(np.uint32)
    sid = np.where(rng.random(npair) < 0.05, rng.choice(np.array(R.NR_X86_64)), rng.integers(0, 30, npair)).astype(np.uint16)
    mn = rng.integers(1, containers + 1, npair).astype(np.uint64) + np.uint64(4026531840)
    mono = np.repeat(ts, 2)[:ns]
    typ = np.tile(np.array([0, 1], np.uint8), npair)[:ns]
    typ[rng.random(ns) < 0.02] = 2
    col = dict(mono_ts=mono, typ=typ, id=np.repeat(sid, 2)[:ns], pid=np.repeat(pid, 2)[:ns])
    # rows arrive roughly in time order with local disorder (several rings); exits a little later
    order = np.argsort(np.arange(ns) + rng.integers(0, 50, ns), kind="stable")
    lost = rng.random(ns) < 0.03
    order = order[~lost[order]] if ns > 8 else order
    col = {k: v[order] for k, v in col.items()}
    n1 = len(order)
    boot = col["mono_ts"] + np.uint64(5_000_000) + rng.integers(0, 3, n1).astype(np.uint64)
    col["sort_ts"] = boot if sort == "boot" else col["mono_ts"].copy()
    mns = np.repeat(mn, 2)[:ns][order]
    pick = rng.integers(0, max(1, n1), nc) if n1 else np.zeros(0, np.int64)
    nc = len(pick)
    col["c_mono_ts"] = col["mono_ts"][pick] if n1 else np.zeros(0, np.uint64)
    col["c_index"] = rng.integers(0, 8, nc).astype(np.uint8)
    if containers > 1:
        col["mntns"] = mns
        col["c_mntns"] = mns[pick] if n1 else np.zeros(0, np.uint64)
    if masks:
        col["valid"] = (rng.random(n1) >= 0.1).astype(np.uint8)
        col["c_valid"] = (rng.random(nc) >= 0.1).astype(np.uint8)
    return col


def test_tile_edges(igx):
    T = igx.engine.traceloop_tile()
    for ns in (0, 1, T - 1, T, T + 1, 2 * T + 1):
        for nc in (0, ns // 2):
            col = stream(ns, nc, seed=ns % 11 + nc % 3, collide=0.3)
            # the generator loses a few rows; top the stream up to exactly ns rows
            short = ns - len(col["mono_ts"])
            if short:
                for k in ("mono_ts", "sort_ts", "typ", "id", "pid"):
                    col[k] = np.concatenate([col[k], col[k][:short]])
            assert len(col["mono_ts"]) == ns and len(col["c_mono_ts"]) == (nc if ns else 0)
            want, _ = check(igx, col)
            assert ns < T - 1 or len(want[0]) > ns // 4


def test_zero_syscall_rows_with_conts(igx):
    col = dict(mono_ts=[], sort_ts=[], typ=[], id=[], pid=[], c_mono_ts=[5, 5, 6], c_index=[0, 1, 0])
    want, _ = check(igx, col)
    assert want[0] == []


def test_one_group_of_three_tiles(igx):
    T = igx.engine.traceloop_tile()
    rng = np.random.default_rng(5)
    ns, nc = 3 * T - 300, 300
    col = dict(mono_ts=np.full(ns, 77, np.uint64), sort_ts=rng.integers(1000, 1050, ns).astype(np.uint64),
               typ=rng.integers(0, 2, ns).astype(np.uint8), id=rng.integers(100, 140, ns).astype(np.uint16),
               pid=rng.integers(1, 40, ns).astype(np.uint32), c_mono_ts=np.full(nc, 77, np.uint64),
               c_index=rng.integers(0, 7, nc).astype(np.uint8))
    col["typ"][:2] = (0, 1)                  # row 0 is e0 and, with row 1 as its exit, m
    col["id"][:2], col["pid"][:2] = 100, 1
    want, _ = check(igx, col)
    # one event completes (m, the group's first row: its conts), every exit is consumed or dropped
    assert want[2].count(0) == 1 and want[2].count(2) == 0 and any(c != R.NO for c in want[3][:6])
    # without any matching exit the whole group is incomplete: every row is an event
    col["pid"] = np.where(col["typ"] == 1, 100, 1).astype(np.uint32)
    want, _ = check(igx, col)
    assert len(want[0]) == ns
    # one exit_group among the enters: it completes alone, the enters are dropped, the exits stay
    col["id"][ns // 2] = 231
    col["typ"][ns // 2] = 0
    want, _ = check(igx, col)
    assert want[2].count(0) == 1 and want[2].count(1) == 0 and want[2].count(2) == int((col["typ"] == 1).sum())


def test_rows_tiles_apart(igx):
    T = igx.engine.traceloop_tile()
    # in the sorted order: e0 = m is the group's last syscall row, behind 2.5 T unmatched enters of
    # a smaller pid (all dropped because of it), and the conts come after everything
    k = 5 * T // 2
    col = dict(mono_ts=np.full(k + 2, 9, np.uint64), sort_ts=np.arange(k + 2, dtype=np.uint64),
               typ=np.array([0] + [0] * k + [1], np.uint8), id=np.array([5] + [1] * k + [5], np.uint16),
               pid=np.array([900] + [1] * k + [900], np.uint32), c_mono_ts=[9, 9, 9], c_index=[1, 0, 1])
    want, _ = check(igx, col)
    assert (want[0], want[1], want[2], want[3]) == ([0], [k + 1], [0], [1, 0] + [R.NO] * 4)
    # in the stream: T enters, two tiles of other timestamps, then their exits
    pid = np.arange(1, T + 1, dtype=np.uint32)
    fill = stream(2 * T, 0, seed=3)
    f = len(fill["mono_ts"])
    col = dict(mono_ts=np.concatenate([np.full(T, 9, np.uint64), fill["mono_ts"], np.full(T, 9, np.uint64)]),
               typ=np.concatenate([np.zeros(T, np.uint8), fill["typ"], np.ones(T, np.uint8)]),
               id=np.concatenate([np.full(T, 3, np.uint16), fill["id"], np.full(T, 3, np.uint16)]),
               pid=np.concatenate([pid, fill["pid"], pid[::-1]]))
    col["sort_ts"] = col["mono_ts"] + np.uint64(1)
    want, _ = check(igx, col)
    assert (want[0][0], want[1][0], want[2][0]) == (0, 2 * T + f - 1, 0)   # only the first enter completes


@pytest.mark.parametrize("containers", [1, 300])
@pytest.mark.parametrize("sort", ["boot", "mono"])
def test_random_streams(igx, containers, sort):
    col = stream(50_000, 12_000, seed=containers + (sort == "mono"), containers=containers, masks=True, sort=sort)
    want, _ = check(igx, col, sync=(sort == "boot"))
    cls = np.asarray(want[2])
    assert (cls == 0).sum() > 10_000 and (cls == 1).sum() > 100 and (cls == 2).sum() > 100
    assert sum(1 for c in want[3] if c != R.NO) > 500


def test_arm64_numbers(igx):
    col = stream(5000, 500, seed=9)
    check(igx, col, nr=R.NR_ARM64)


def test_two_calls_identical_bytes(igx):
    col = stream(30_000, 6_000, seed=17, containers=20, masks=True)
    _, n1, a = device_join(igx, col, sync=False)
    _, n2, b = device_join(igx, col, sync=False)
    assert n1 == n2
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["row"][n1:] == -1).all() and (a["cls"][n1:] == 0xFF).all()


def test_argument_errors_on_a_live_context(igx, torch):
    ctx = igx.runtime.context()
    L, EINVAL = ctx.L, igx._abi.IGX_EINVAL
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    vp = C.c_void_p

    def call(mntns=None, mono=p, sort=p, typ=p, id=p, pid=p, ns=16, c_mntns=None, c_mono=p, c_index=p, nc=4,
             row=p + 8192, ex=p + 12288, cls=p + 16384, cont=p + 20480, nev=p + 28672):
        return L.igx_traceloop_join(ctx.h, vp(mntns), vp(mono), vp(sort), vp(typ), vp(id), vp(pid), None, ns,
                                    vp(c_mntns), vp(c_mono), vp(c_index), None, nc, 60, 231, 15, vp(row), vp(ex),
                                    vp(cls), vp(cont), vp(nev))

    assert call() == 0
    assert call(ns=0xFFFFFFFF) == EINVAL and call(ns=0xFFFFFFF0, nc=0x10) == EINVAL
    assert call(nev=None) == EINVAL and call(nev=p + 28676) == EINVAL
    assert call(mono=None) == EINVAL and call(row=None) == EINVAL and call(c_index=None) == EINVAL
    assert call(mntns=p) == EINVAL and call(c_mntns=p) == EINVAL           # mntns on one stream only
    assert call(mono=p + 4) == EINVAL and call(sort=p + 4) == EINVAL and call(c_mono=p + 4) == EINVAL
    assert call(pid=p + 2) == EINVAL and call(id=p + 1) == EINVAL
    assert call(row=p + 8194) == EINVAL and call(ex=p + 12290) == EINVAL and call(cont=p + 20482) == EINVAL
    assert call(mntns=p, c_mntns=p) == 0 and call(nc=0, c_mono=None, c_index=None) == 0
    assert "traceloop_join" in L.igx_last_error(ctx.h).decode()
    torch.cuda.synchronize()


def test_conts_beside_rows_of_pid_zero(igx):
    """The sort key files the conts of parameter i beside syscall rows of pid 0 and id i (the idle
    task's number): such rows keep their own matches and the conts stay conts."""
    col = dict(mono_ts=[9] * 6, sort_ts=[1, 2, 3, 4, 5, 6], typ=[0, 0, 1, 1, 0, 1], id=[1, 0, 0, 1, 5, 5],
               pid=[0, 0, 0, 0, 0, 7], c_mono_ts=[9, 9, 9, 9], c_index=[1, 0, 5, 1])
    want, _ = check(igx, col)
    assert (want[0], want[1], want[2], want[3]) == ([0], [3], [0], [1, 0, R.NO, R.NO, R.NO, 2])
    col["valid"] = [0, 1, 1, 1, 1, 1]
    want, _ = check(igx, col)
    assert (want[0], want[1], want[3][:2]) == ([1], [2], [1, 0])
