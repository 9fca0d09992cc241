"""igx_req_join (the block-I/O start / issue / done pairing on the device) against the sequential
restatement in tests/reqjoin_ref.py: all four output arrays, both counts and the live rows, bit
for bit; then the two gadgets that use it against their delta-fed forms.

Sizes: the contract's hand cases; 0, 1 and the scan tile - 1 / tile / tile + 1 rows (the tile comes
from the library); one request for 70 000 rows (a run across many tiles and workgroups) and
70 000 distinct requests; 200 000 rows over 64 requests that differ in byte 7 only, and in byte 0
only (the sort's digit plan at both ends); START-heavy, DONE-only and D D I D D streams; a nil
mask; kinds 3 and 255; wrapping deltas; pend_cap below the live count; the row limit."""
import ctypes as C

import numpy as np
import pytest

import reqjoin_ref as R

pytestmark = pytest.mark.gpu


def _device_join(igx, req, kind, ts, valid=None, pend_cap=None):
    H = igx.columns
    j = igx.engine.req_join(H.to_device(req), H.to_device(kind), H.to_device(ts),
                            None if valid is None else H.to_device(valid), pend_cap=pend_cap)
    got = {k: H.host(j[k]) for k in ("done", "issue", "who", "delta", "pend")}
    for k in ("done", "issue", "who", "pend"):
        got[k] = got[k].view(np.uint32)
    return got, j["n_done"], j["n_pend"]


def _check(igx, req, kind, ts, valid=None):
    done, issue, who, delta, live = R.join_arrays(req, kind, ts, valid)
    got, nd, npend = _device_join(igx, req, kind, ts, valid)
    assert nd == len(done) and npend == len(live)
    assert np.array_equal(got["done"], done)
    assert np.array_equal(got["issue"], issue)
    assert np.array_equal(got["who"], who)
    assert np.array_equal(got["delta"], delta)
    assert np.array_equal(got["pend"], live)
    return done, live, delta


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(igx, case):
    _, req, kind, ts, emitted, live = case
    got, nd, npend = _device_join(igx, req, kind, ts)
    assert [tuple(int(x) for x in t) for t in zip(got["done"], got["issue"], got["who"])] == emitted
    assert list(got["pend"]) == live and nd == len(emitted) and npend == len(live)
    _check(igx, req, kind, ts)


def test_tile_edges(igx):
    tile = igx.engine.req_join_tile()
    for n in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 5):
        req, kind, ts = R.random_stream(n, 5, seed=100 + n % 7) if n else \
            (np.zeros(0, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint64))
        done, _, _ = _check(igx, req, kind, ts)
        assert n < tile - 1 or len(done) > 100


def test_one_request_many_tiles(igx):
    n = 70_000
    _, kind, ts = R.random_stream(n, 1, seed=3)
    req = np.full(n, 0xFFFF8881234567C0, np.uint64)
    done, _, _ = _check(igx, req, kind, ts)
    assert len(done) > 5000


def test_all_distinct_requests(igx):
    n = 70_000
    _, kind, ts = R.random_stream(n, 1, seed=4)
    req = np.uint64(0xFFFF888000000000) + np.random.default_rng(4).permutation(n).astype(np.uint64) * np.uint64(64)
    done, live, _ = _check(igx, req, kind, ts)
    assert len(done) == 0 and len(live) == int((kind != R.DONE).sum())


@pytest.mark.parametrize("shift", [56, 0], ids=["byte7", "byte0"])
def test_requests_differ_in_one_byte(igx, shift):
    n = 200_000
    rng = np.random.default_rng(shift + 1)
    _, kind, ts = R.random_stream(n, 1, seed=5 + shift)
    ids = rng.permutation(256)[:64].astype(np.uint64)
    base = np.uint64(0x00FF888812345600) if shift == 56 else np.uint64(0xFFFF888812345600)
    req = base + (ids[rng.integers(0, 64, n)] << np.uint64(shift))
    done, _, _ = _check(igx, req, kind, ts)
    assert len(done) > 20_000


@pytest.mark.parametrize("mix", ["start-heavy", "done-only", "ddidd"])
def test_adversarial_mixes(igx, mix):
    n = 30_000
    req, kind, ts = R.random_stream(n, 7, seed=21, p_kind=(0.9, 0.05, 0.05))
    if mix == "done-only":
        kind[:] = R.DONE
    elif mix == "ddidd":
        kind = np.tile(np.array([R.DONE, R.DONE, R.ISSUE, R.DONE, R.DONE], np.uint8), n // 5)
        req = np.repeat(req[: n // 5], 5)          # each D D I D D on one request, requests interleaved in blocks
    done, live, _ = _check(igx, req, kind, ts)
    if mix == "done-only":
        assert len(done) == 0 and len(live) == 0
    else:
        assert len(done) > 100


def test_valid_mask(igx):
    n = 50_000
    req, kind, ts = R.random_stream(n, 300, seed=31)
    valid = (np.random.default_rng(32).random(n) >= 0.3).astype(np.uint8)
    done, live, delta = _check(igx, req, kind, ts, valid)
    # the same as joining the surviving rows alone, with their ids mapped back
    keep = np.flatnonzero(valid)
    d2, i2, w2, dl2, l2 = R.join_arrays(req[keep], kind[keep], ts[keep])
    assert np.array_equal(keep[d2], done) and np.array_equal(keep[l2], live) and np.array_equal(dl2, delta)


def test_other_kinds_are_ignored(igx):
    n = 20_000
    req, kind, ts = R.random_stream(n, 50, seed=41)
    rng = np.random.default_rng(42)
    kind[rng.random(n) < 0.15] = 3
    kind[rng.random(n) < 0.15] = 255
    done, _, _ = _check(igx, req, kind, ts)
    assert len(done) > 1000


def test_wrapping_deltas(igx):
    req, kind, ts = R.random_stream(20_000, 50, seed=51, wrap_ts=True)
    ts[::3] = ts[::3][::-1].copy()
    _, _, delta = _check(igx, req, kind, ts)
    neg = int((delta >= np.uint64(1 << 63)).sum())
    assert 100 < neg < len(delta) - 100


def test_pend_cap_below_live_count(igx, torch):
    H = igx.columns
    n, cap = 10_000, 37
    req, kind, ts = R.random_stream(n, 4000, seed=61, p_kind=(0.5, 0.4, 0.1))
    _, _, _, _, live = R.join_arrays(req, kind, ts)
    assert len(live) > 10 * cap
    ctx = igx.runtime.context()
    d = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    delta = torch.empty(n, dtype=torch.uint64, device="cuda")
    pend = torch.full((cap + 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    p = igx.runtime.ptr
    t = [H.to_device(x) for x in (req, kind, ts)]
    ctx.check(ctx.L.igx_req_join(ctx.h, p(t[0]), p(t[1]), p(t[2]), None, n, p(d[0]), p(d[1]), p(d[2]), p(delta),
                                 C.c_void_p(cnt.data_ptr()), p(pend), cap, C.c_void_p(cnt.data_ptr() + 8)))
    got = pend.cpu().numpy().view(np.uint32)
    assert int(cnt[1]) == len(live)
    assert np.array_equal(got[:cap], live[:cap])
    assert np.all(got[cap:] == 0x5A5A5A5A)


def test_row_limit(igx):
    """nrows = 2^32 - 1 is refused before any argument is looked at (the pointers are null)."""
    ctx = igx.runtime.context()
    rc = ctx.L.igx_req_join(ctx.h, None, None, None, None, (1 << 32) - 1, None, None, None, None, None, None, 0, None)
    assert rc == igx._abi.IGX_EINVAL
    assert b"rows" in ctx.L.igx_last_error(ctx.h)


# ---- the gadgets ------------------------------------------------------------------------------
def _probe_stream(n, seed, with_start=True):
    """A block-I/O probe stream: request pointers from a pool of 400, per-row attributes of
    small cardinality so that the joined rows fall into a few hundred groups."""
    rng = np.random.default_rng(seed)
    req, kind, ts = R.random_stream(n, 400, seed, p_kind=(0.32, 0.34, 0.34) if with_start else (0.0, 0.5, 0.5))
    comm = np.zeros((n, 16), np.uint8)
    names = [b"fio", b"postgres", b"jbd2/sda1-8", b"kworker/u8:3"]
    for i, c in enumerate(rng.integers(0, len(names), n)):
        comm[i, :len(names[c])] = np.frombuffer(names[c], np.uint8)
    return {"req": req, "kind": kind, "ts": ts,
            "mntns": (np.uint64(4026531840) + rng.integers(0, 3, n).astype(np.uint64)),
            "pid": rng.integers(100, 120, n).astype(np.uint32), "comm": comm,
            "data_len": (rng.integers(1, 64, n) * 4096).astype(np.uint64),
            "cmd_flags": (rng.integers(0, 3, n) | (rng.integers(0, 4, n) << 11)).astype(np.uint32),
            "major": rng.choice(np.array([8, 259], np.int32), n), "minor": rng.integers(0, 3, n).astype(np.int32)}


def _emitted_by_batch(ev, cuts, valid=None):
    """The restatement's emitted rows, grouped by the batch whose DONE row emitted them: per
    batch (done, issue, who as int64 global rows; delta as uint64)."""
    em, _ = R.join_batches(ev["req"], ev["kind"], ev["ts"], cuts, valid)
    bounds = list(cuts) + [len(ev["req"])]
    out = [[] for _ in bounds]
    for e in em:
        out[int(np.searchsorted(bounds, e[0], side="right"))].append(e)
    return [(np.array([e[0] for e in b], np.int64), np.array([e[1] for e in b], np.int64),
             np.array([e[2] for e in b], np.int64), np.array([e[3] for e in b], np.uint64)) for b in out]


def test_top_block_io_from_probes(igx, torch):
    G, H = igx.gadgets, igx.columns
    n, cuts = 150_000, (41_003, 97_001)
    ev = _probe_stream(n, 71)
    bounds = [0] + list(cuts) + [n]
    tr = G.TopBlockIOProbeTracer(capacity=1 << 14)
    ref = G.TopBlockIOTracer(capacity=1 << 14)
    per_batch = _emitted_by_batch(ev, cuts)
    assert all(len(b[0]) > 5000 for b in per_batch)
    intervals = []
    for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        tr.feed({k: H.to_device(v[lo:hi]) for k, v in ev.items()})
        d, i, w, delta = per_batch[b]
        has = w != R.NONE
        ws = np.where(has, w, 0)
        joined = {"mntns": np.where(has, ev["mntns"][ws], 0).astype(np.uint64),
                  "pid": np.where(has, ev["pid"][ws], 0).astype(np.uint32),
                  "comm": np.where(has[:, None], ev["comm"][ws], 0).astype(np.uint8),
                  "rwflag": np.array([G.rwflag_of(x) for x in ev["cmd_flags"][d]], np.int32),
                  "major": ev["major"][d], "minor": ev["minor"][d], "data_len": ev["data_len"][i],
                  "delta_ns": delta}
        ref.feed({k: H.to_device(v) for k, v in joined.items()})
        if b >= 1:        # requests straddle the batch boundary inside interval 1 and the interval boundary after it
            assert tr.pending > 0
            got, want = tr.nextStats(), ref.nextStats()
            assert len(want) > 100 and got == want
            intervals.append(got)
    assert any(s.Pid == 0 and s.Comm == "" for s in intervals[0])       # DONEs without a START entry
    tr.destroy()
    ref.destroy()


def test_pending_cap_exceeded_raises(igx):
    G, H = igx.gadgets, igx.columns
    ev = _probe_stream(600, 91)
    ev["req"] = np.uint64(0xFFFF888000000000) + np.arange(600, dtype=np.uint64) * np.uint64(64)
    ev["kind"][:] = R.START                                  # 600 requests in flight
    tr = G.TopBlockIOProbeTracer(pending_cap=100, capacity=1 << 10)
    with pytest.raises(igx.IgxError, match="pending_cap=100") as e:
        tr.feed({k: H.to_device(v) for k, v in ev.items()})
    assert e.value.code == igx._abi.IGX_ENOSPC and "600 requests" in str(e.value)
    tr.destroy()


@pytest.mark.parametrize("per_disk", [False, True], ids=["plain", "per_disk"])
def test_profile_block_io_from_probes(igx, torch, per_disk):
    G, H = igx.gadgets, igx.columns
    n, cuts = 60_000, (25_001,)
    ev = _probe_stream(n, 81, with_start=False)
    ev["ts"][::5] = ev["ts"][::5][::-1].copy()            # planted: some completions "before" their issue
    dev = (ev["major"].astype(np.uint32) << np.uint32(20)) | ev["minor"].astype(np.uint32)
    bounds = [0] + list(cuts) + [n]
    tr, ref = G.ProfileBlockIOTracer(per_disk=per_disk), G.ProfileBlockIOTracer(per_disk=per_disk)
    neg = 0
    per_batch = _emitted_by_batch(ev, cuts)
    for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        tr.feed_probes(*(H.to_device(ev[k][lo:hi]) for k in ("req", "kind", "ts")), dev=H.to_device(dev[lo:hi]),
                       cmd_flags=H.to_device(ev["cmd_flags"][lo:hi]))
        d, _, _, delta = per_batch[b]
        delta = delta.view(np.int64)
        neg += int((delta < 0).sum())
        ref.feed(H.to_device(delta), dev=H.to_device(dev[d]), cmd_flags=H.to_device(ev["cmd_flags"][d]))
    assert neg > 100
    assert np.array_equal(tr.slots(), ref.slots()) and tr.slots().sum() > 5000
    assert tr.keys() == ref.keys() and (len(tr.keys()) == 6) == per_disk
