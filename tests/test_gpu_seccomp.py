"""igx_seccomp_* on the device against the row-by-row restatement of ig_seccomp_e
(tests/seccomp_ref.py), bit for bit.  Every case compares the 501-byte values and the found
bytes of all namespaces fed, of one never fed and of namespace 0.  Row counts around the kernels'
tiles, slot contention, capacity and overflow, colliding home slots, the drop rules, comm and
arg0 edge values, the gate in every position, batch-cut invariance, delete, and both mark forms
either side of the LDS threshold."""
import ctypes as C

import numpy as np
import pytest

from seccomp_ref import SeccompRef

pytestmark = pytest.mark.gpu

PRCTL, SECCOMP = 157, 317
RUNC, INIT, SH = b"runc", b"runc:[2:INIT]", b"sh"
GATE_TILE = 256         # rows per workgroup pass of the gate launch (k_seccomp.hip TB)
GLOBAL_TILE = 1024      # ... of the global mark form (TB x CPL)
LDS_TILE = 4096         # ... of the LDS mark form (TBL x CPL)
LDS_CAP = 1024          # the largest capacity marked through LDS: S = 2048 slots
NEVER = 0xDEAD0000BEEF  # a namespace no stream holds


def stream(rows):
    """Columns of hand-written rows (mntns, id, arg0, comm[, compat])."""
    n = len(rows)
    comm = np.zeros((n, 16), np.uint8)
    for i, r in enumerate(rows):
        comm[i, :len(r[3])] = np.frombuffer(r[3], np.uint8)
    return {"mntns": np.array([r[0] for r in rows], np.uint64), "id": np.array([r[1] for r in rows], np.uint32),
            "arg0": np.array([r[2] for r in rows], np.uint64), "comm": comm,
            "compat": np.array([r[4] if len(r) > 4 else 0 for r in rows], np.uint8)}


def rand_stream(rng, n, pool, runc=0.3):
    """n rows over the namespaces of pool: runc rows mix arming, excluded and ordinary calls."""
    pool = np.asarray(pool, np.uint64)
    is_runc = rng.random(n) < runc
    k = rng.integers(0, 10, n)
    ids = rng.integers(0, 500, n).astype(np.uint32)
    ids[is_runc & (k < 3)] = PRCTL
    ids[is_runc & (k == 3)] = SECCOMP
    arg0 = rng.choice(np.array([2, 38, 0, 7, 2 + (1 << 32)], np.uint64), n, p=[0.15, 0.2, 0.3, 0.3, 0.05])
    comm = np.zeros((n, 16), np.uint8)
    comm[:, :2] = np.frombuffer(SH, np.uint8)
    comm[is_runc, :len(INIT)] = np.frombuffer(INIT, np.uint8)
    return {"mntns": pool[rng.integers(0, len(pool), n)], "id": ids, "arg0": arg0, "comm": comm,
            "compat": np.zeros(n, np.uint8)}


def cut(s, a, b):
    return {k: v[a:b] for k, v in s.items()}


def feed(igx, m, ref, s, valid=None, use_compat=True, to_ref=True):
    D = igx.columns.to_device
    m.update(D(s["mntns"]), D(s["id"]), D(s["arg0"]), D(s["comm"]), D(s["compat"]) if use_compat else None,
             None if valid is None else D(np.asarray(valid, np.uint8)))
    if to_ref and ref is not None:
        ref.feed(s["mntns"], s["id"], s["arg0"], s["comm"], s["compat"] if use_compat else None, valid)


def check(m, ref, keys, tag=""):
    """Values and found bytes of keys, a namespace never fed and namespace 0, and the entries."""
    keys = sorted({int(k) for k in keys} | {NEVER, 0})
    val, found = m.peek(keys)
    for i, k in enumerate(keys):
        want = ref.lookup(k)
        assert bool(found[i]) == (want is not None), (tag, hex(k), "found")
        assert val[i].tobytes() == (want or bytes(501)), (tag, hex(k), np.flatnonzero(val[i]).tolist(),
                                                          [j for j, b in enumerate(want or b"") if b])
    live = sorted(k for k in ref.map if k != 0)
    assert m.count() == len(live), tag
    assert m.list().tolist() == live, tag


@pytest.fixture
def mk(igx):
    made = []

    def make(capacity=LDS_CAP, nr=(PRCTL, SECCOMP)):
        m = igx.engine.SeccompMap(capacity, *nr)
        made.append(m)
        return m, SeccompRef(*nr)
    yield make
    for m in made:
        m.destroy()


@pytest.mark.parametrize("capacity", [LDS_CAP, 2 * LDS_CAP], ids=["lds", "global"])
def test_row_counts(igx, mk, capacity):
    rng = np.random.default_rng(capacity)
    m, ref = mk(capacity)
    pool = rng.integers(1, 1 << 40, 40)
    for n in (0, 1, 63, 64, 65, GATE_TILE - 1, GATE_TILE, GATE_TILE + 1, GLOBAL_TILE - 1, GLOBAL_TILE, GLOBAL_TILE + 1,
              LDS_TILE - 1, LDS_TILE, LDS_TILE + 1):
        feed(igx, m, ref, rand_stream(rng, n, pool))
        check(m, ref, pool, n)


@pytest.mark.parametrize("capacity", [LDS_CAP, 2 * LDS_CAP], ids=["lds", "global"])
def test_one_namespace_for_every_row(igx, mk, capacity):
    rng = np.random.default_rng(3)
    m, ref = mk(capacity)
    feed(igx, m, ref, rand_stream(rng, 70001, [4026532000]))
    check(m, ref, [4026532000])


@pytest.mark.parametrize("capacity", [LDS_CAP, 2 * LDS_CAP], ids=["lds", "global"])
def test_1024_namespaces_uniform_at_exact_capacity(igx, mk, capacity):
    rng = np.random.default_rng(4)
    pool = np.unique(rng.integers(1, 1 << 63, 2 * capacity).astype(np.uint64))[:capacity]
    assert len(pool) == capacity
    s = rand_stream(rng, 40000, pool)
    s["mntns"][:capacity] = pool           # every namespace appears: exactly capacity distinct
    m, ref = mk(capacity)
    feed(igx, m, ref, s)
    check(m, ref, pool)
    assert m.count() == capacity


@pytest.mark.parametrize("capacity", [5, LDS_CAP, LDS_CAP + 1], ids=["5", "lds", "global"])
def test_overflow(igx, mk, capacity):
    rng = np.random.default_rng(5)
    pool = np.arange(1000, 1000 + capacity + 1, dtype=np.uint64)
    m, ref = mk(capacity)
    s = rand_stream(rng, 3 * (capacity + 1), pool[:capacity])
    s["mntns"][:capacity] = pool[:capacity]
    feed(igx, m, ref, s)
    check(m, ref, pool[:capacity])                     # full, not over
    s = rand_stream(rng, 100, pool)
    s["mntns"][17] = pool[capacity]                    # one namespace too many
    feed(igx, m, None, s)
    for _ in range(2):
        with pytest.raises(igx._abi.IgxError) as e:
            m.count()
        assert e.value.code == igx._abi.IGX_ENOSPC
    with pytest.raises(igx._abi.IgxError) as e:
        m.list()
    assert e.value.code == igx._abi.IGX_ENOSPC
    with pytest.raises(igx._abi.IgxError) as e:        # later feeds are refused
        feed(igx, m, None, rand_stream(rng, 10, pool[:2]))
    assert e.value.code == igx._abi.IGX_ENOSPC
    m.destroy()
    m.destroy()                                        # and destroy works, twice


def test_deleted_namespaces_count_against_capacity(igx, mk):
    m, ref = mk(4)
    feed(igx, m, ref, stream([(k, 1, 0, SH) for k in (11, 12, 13, 14)]))
    m.delete([11, 12])
    ref.delete(11), ref.delete(12)
    check(m, ref, [11, 12, 13, 14])
    feed(igx, m, ref, stream([(11, 2, 0, SH)]))       # its own slot again: still four keys
    check(m, ref, [11, 12, 13, 14])
    feed(igx, m, None, stream([(15, 2, 0, SH)]))      # a fifth key
    with pytest.raises(igx._abi.IgxError) as e:
        m.count()
    assert e.value.code == igx._abi.IGX_ENOSPC


@pytest.mark.parametrize("capacity", [LDS_CAP, 2 * LDS_CAP], ids=["lds", "global"])
def test_chain_of_keys_sharing_a_home_slot(igx, mk, capacity):
    m, ref = mk(capacity)
    S = m.slots()
    assert S == 2 * capacity
    chain, k = [], 1
    while len(chain) < 8:                              # eight namespaces whose probes start at the last slot
        if igx.engine.seccomp_home(k, S) == S - 1:     # so the chain wraps round to slot 0
            chain.append(k)
        k += 1
    rng = np.random.default_rng(6)
    others = rng.integers(1 << 40, 1 << 41, 50)
    feed(igx, m, ref, rand_stream(rng, 5000, chain + list(others)))
    check(m, ref, chain + list(others))
    m.delete([chain[3]])
    ref.delete(chain[3])
    check(m, ref, chain + list(others), "deleted")     # those behind it in the chain are still found
    feed(igx, m, ref, rand_stream(rng, 3000, chain))
    check(m, ref, chain + list(others), "re-fed")


def test_drop_rules_and_valid_mask(igx, mk):
    m, ref = mk()
    rows = [(7, 0, 0, SH), (7, 499, 0, SH), (7, 500, 0, SH), (7, 0xFFFFFFFF, 0, SH),
            (8, 500, 0, SH),                      # only dropped rows: no entry
            (9, 5, 0, SH, 1),                     # compat: no entry
            (0, 5, 0, SH), (0, PRCTL, 2, RUNC),   # mntns 0
            (10, 6, 0, SH, 255), (10, 7, 0, SH),  # any non-zero compat byte drops
            (11, 8, 0, SH), (11, 9, 0, SH)]
    valid = [1] * len(rows)
    valid[-1] = 0
    feed(igx, m, ref, stream(rows), valid=valid)
    check(m, ref, [7, 8, 9, 10, 11])
    assert ref.lookup(8) is None and ref.lookup(9) is None and ref.lookup(11)[9] == 0
    # no compat column is compat 0; a masked arming row does not arm
    m, ref = mk()
    rows = [(7, PRCTL, 2, RUNC), (7, 60, 0, RUNC), (8, PRCTL, 2, RUNC), (8, 61, 0, RUNC)]
    feed(igx, m, ref, stream(rows), valid=[0, 1, 1, 1], use_compat=False)
    check(m, ref, [7, 8])
    assert ref.lookup(7)[500] == 0 and ref.lookup(8)[61] == 1


def test_comm_values(igx, mk):
    m, ref = mk()
    comms = [RUNC, INIT, b"run", b"runx", b"Runc", b"runcABCDEFGHIJKL", b"RUNC", b"xrunc", b""]
    rows = [(100 + i, PRCTL, 2, c) for i, c in enumerate(comms)] + [(100 + i, 42, 0, c) for i, c in enumerate(comms)]
    feed(igx, m, ref, stream(rows))
    check(m, ref, range(100, 100 + len(comms)))
    assert [ref.lookup(100 + i)[500] for i in range(len(comms))] == [1, 1, 0, 0, 0, 1, 0, 0, 0]
    # a comm column with a row stride of 24 and one of 4 bytes, and an unaligned one
    D = igx.columns.to_device
    s = stream(rows)
    for view in ("wide", "narrow", "odd"):
        m, ref = mk()
        if view == "wide":
            buf = np.full((len(rows), 24), 0x72, np.uint8)
            buf[:, :16] = s["comm"]
            comm = D(buf)[:, :16]
        elif view == "narrow":
            comm = D(s["comm"][:, :4].copy())
        else:
            buf = np.full(len(rows) * 17 + 1, 0x72, np.uint8)
            buf[1:].reshape(len(rows), 17)[:, :16] = s["comm"]
            comm = D(buf)[1:].view(len(rows), 17)[:, :16]
        m.update(D(s["mntns"]), D(s["id"]), D(s["arg0"]), comm)
        ref.feed(s["mntns"], s["id"], s["arg0"], s["comm"])
        check(m, ref, range(100, 100 + len(comms)), view)


def test_arg0_high_bits_do_not_match(igx, mk):
    m, ref = mk()
    hi = 1 << 32
    rows = [(7, PRCTL, 2 + hi, RUNC), (7, 60, 0, RUNC),          # not armed by 2 + 2^32
            (8, PRCTL, 2, RUNC), (8, PRCTL, 38 + hi, RUNC),      # 38 + 2^32 is recorded as a prctl
            (9, PRCTL, 2, RUNC), (9, PRCTL, 38, RUNC),           # the real one is not
            (10, PRCTL, (1 << 63) + 2, RUNC), (10, 61, 0, RUNC)]
    feed(igx, m, ref, stream(rows))
    check(m, ref, [7, 8, 9, 10])
    assert ref.lookup(7) == bytes(501) and ref.lookup(8)[PRCTL] == 1 and ref.lookup(9)[PRCTL] == 0


@pytest.mark.parametrize("capacity", [LDS_CAP, 2 * LDS_CAP], ids=["lds", "global"])
def test_gate_cases(igx, mk, capacity):
    A, B = 4026531840, 4026532111
    # the arming row is the first row of the stream
    m, ref = mk(capacity)
    feed(igx, m, ref, stream([(A, PRCTL, 2, INIT), (A, 59, 0, INIT), (A, 60, 0, INIT)]))
    check(m, ref, [A], "first")
    assert ref.lookup(A)[59] == 1 and ref.lookup(A)[PRCTL] == 0
    # the arming row is the last row of a batch, the gated rows are in the next
    m, ref = mk(capacity)
    feed(igx, m, ref, stream([(A, 56, 0, INIT), (A, 57, 0, INIT), (A, PRCTL, 2, INIT)]))
    check(m, ref, [A], "armed at the end")
    feed(igx, m, ref, stream([(A, 59, 0, INIT), (A, 1, 0, INIT)]))
    check(m, ref, [A], "next batch")
    assert ref.lookup(A)[59] == 1 and ref.lookup(A)[56] == 0
    # two arming rows: the second is recorded as a prctl
    m, ref = mk(capacity)
    feed(igx, m, ref, stream([(A, PRCTL, 2, INIT), (A, 3, 0, INIT), (A, PRCTL, 2, INIT)]))
    check(m, ref, [A], "two arms")
    assert ref.lookup(A)[PRCTL] == 1
    # ... and across a batch cut; an arming row in A leaves B unarmed
    m, ref = mk(capacity)
    feed(igx, m, ref, stream([(A, PRCTL, 2, INIT), (B, 3, 0, INIT)]))
    feed(igx, m, ref, stream([(A, PRCTL, 2, INIT), (B, 4, 0, INIT), (A, 5, 0, INIT)]))
    check(m, ref, [A, B], "A not B")
    assert ref.lookup(B) == bytes(501) and ref.lookup(A)[PRCTL] == 1
    # the excluded prctl(38) and seccomp before and after arming
    m, ref = mk(capacity)
    feed(igx, m, ref, stream([(A, PRCTL, 38, INIT), (A, SECCOMP, 0, INIT), (A, PRCTL, 2, INIT), (A, PRCTL, 38, INIT),
                              (A, SECCOMP, 1, INIT), (A, 9, 0, INIT), (B, SECCOMP, 0, INIT), (B, PRCTL, 38, RUNC)]))
    check(m, ref, [A, B], "excluded")
    assert [j for j, b in enumerate(ref.lookup(A)) if b] == [9, 500] and ref.lookup(B) == bytes(501)
    # only pre-gate runc rows: found, all 501 bytes zero; a non-runc row before the gate is recorded
    m, ref = mk(capacity)
    feed(igx, m, ref, stream([(A, 1, 0, RUNC), (A, 2, 0, RUNC), (B, 7, 0, SH), (B, 8, 0, RUNC), (B, PRCTL, 2, RUNC),
                              (B, 9, 0, RUNC), (B, 10, 0, SH)]))
    check(m, ref, [A, B], "pre-gate")
    assert ref.lookup(A) == bytes(501)
    assert [j for j, b in enumerate(ref.lookup(B)) if b] == [7, 9, 10, 500]
    # arm64's numbers
    m, ref = mk(capacity, nr=(167, 277))
    feed(igx, m, ref, stream([(A, 157, 2, INIT), (A, 167, 2, INIT), (A, 277, 0, INIT), (A, 157, 2, INIT)]))
    check(m, ref, [A], "arm64")


@pytest.mark.parametrize("capacity", [LDS_CAP, 2 * LDS_CAP], ids=["lds", "global"])
def test_batch_cut_invariance(igx, mk, capacity):
    rng = np.random.default_rng(8)
    n = 1 << 18
    pool = rng.integers(1, 1 << 48, 1024)
    s = rand_stream(rng, n, pool, runc=0.2)
    whole, ref = mk(capacity)
    feed(igx, whole, ref, s)
    check(whole, ref, pool, "whole")
    parts, _ = mk(capacity)
    cuts = [0] + sorted(rng.integers(1, n, 7).tolist()) + [n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        feed(igx, parts, None, cut(s, a, b))
    check(parts, ref, pool, cuts)


@pytest.mark.parametrize("capacity", [LDS_CAP, 2 * LDS_CAP], ids=["lds", "global"])
def test_delete_then_refeed(igx, mk, capacity):
    rng = np.random.default_rng(9)
    m, ref = mk(capacity)
    pool = [21, 22, 23]
    feed(igx, m, ref, rand_stream(rng, 4000, pool, runc=0.5))
    assert ref.lookup(21)[500] == 1
    m.delete([21, 999, 21, 0])                          # one never fed, one twice, and key 0
    ref.delete(21), ref.delete(999)
    check(m, ref, pool + [999], "deleted")
    feed(igx, m, ref, stream([(21, 70, 0, INIT), (21, 71, 0, SH)]))   # blank again, and no gate
    check(m, ref, pool, "re-fed")
    assert [j for j, b in enumerate(ref.lookup(21)) if b] == [71]
    feed(igx, m, ref, stream([(21, PRCTL, 2, INIT), (21, 70, 0, INIT)]))
    check(m, ref, pool, "re-armed")
    m.delete([])                                        # nothing to do
    val, found = m.peek([])
    assert val.shape == (0, 501) and found.shape == (0,)


def test_both_forms_give_the_same_values(igx, mk):
    """One stream at a capacity on each side of the LDS threshold, at the largest table the LDS
    form takes (S = 2048) and the next power of two (S = 4096), and at small ones."""
    rng = np.random.default_rng(10)
    pool = rng.integers(1, 1 << 48, 900)
    s = rand_stream(rng, 50000, pool)
    ref = None
    for capacity, S in ((LDS_CAP, 2048), (LDS_CAP + 1, 4096), (2 * LDS_CAP, 4096), (900, 2048), (1 << 16, 1 << 17)):
        m, r = mk(capacity)
        assert m.slots() == S
        feed(igx, m, r if ref is None else None, s)
        ref = ref or r
        check(m, ref, pool, capacity)


def test_argument_errors_on_a_live_object(igx, mk, torch):
    L, EINVAL = igx.lib(), igx._abi.IGX_EINVAL
    ctx = igx.runtime.context()
    h = C.c_void_p()
    for cap in (0, (1 << 19) + 1):
        assert L.igx_seccomp_create(ctx.h, cap, PRCTL, SECCOMP, C.byref(h)) == EINVAL and not h.value
    assert L.igx_seccomp_create(ctx.h, 8, PRCTL, SECCOMP, None) == EINVAL
    m, ref = mk(8)
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert L.igx_seccomp_update(m.h, p, p, p, p, 3, None, None, 4) == EINVAL              # comm_stride < 4
    assert L.igx_seccomp_update(m.h, p, p, p, p, 0, None, None, 0) == EINVAL
    for hole in range(4):                                                                # a null column
        cols = [p, p, p, p]
        cols[hole] = None
        assert L.igx_seccomp_update(m.h, *cols, 16, None, None, 4) == EINVAL
    assert L.igx_seccomp_update(m.h, None, None, None, None, 16, None, None, 0) == 0      # no rows: nothing to read
    odd = C.c_void_p(buf.data_ptr() + 4)
    assert L.igx_seccomp_update(m.h, odd, p, p, p, 16, None, None, 4) == EINVAL           # mntns alignment
    assert L.igx_seccomp_update(m.h, p, C.c_void_p(buf.data_ptr() + 2), p, p, 16, None, None, 4) == EINVAL
    assert L.igx_seccomp_update(m.h, p, p, p, p, 16, None, None, 1 << 31) == EINVAL
    assert L.igx_seccomp_peek(m.h, None, 1, p, p) == EINVAL and L.igx_seccomp_peek(m.h, p, 1, None, p) == EINVAL
    assert L.igx_seccomp_delete(m.h, None, 1) == EINVAL
    assert L.igx_seccomp_count(m.h, None) == EINVAL
    n = C.c_uint64()
    assert L.igx_seccomp_list(m.h, None, 4, C.byref(n)) == EINVAL
    check(m, ref, [1])                                                                   # nothing was fed
    feed(igx, m, ref, stream([(1, 1, 0, SH), (2, 2, 0, SH), (3, 3, 0, SH)]))
    assert L.igx_seccomp_list(m.h, None, 0, C.byref(n)) == 0 and n.value == 3            # a count-only list
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert L.igx_seccomp_list(m.h, C.c_void_p(out.data_ptr()), 2, C.byref(n)) == 0 and n.value == 3
    assert set(out.cpu().tolist()) < {1, 2, 3} and len(set(out.cpu().tolist())) == 2      # the first cap of them
