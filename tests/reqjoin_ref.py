"""Sequential restatement of the block-I/O request pairing (include/igx.h, igx_req_join): the two
hash maps of biotop.bpf.c:41-130 (`whobyreq`, `start`) and the one of biolatency.bpf.c:47-154,
keyed by the request pointer, walked row by row with Python dicts.  A helper for the tests of
the device join, not a test module."""
import numpy as np

START, ISSUE, DONE = 0, 1, 2
NONE = 0xFFFFFFFF
U64 = (1 << 64) - 1


def join(req, kind, ts, valid=None):
    """One batch.  Returns (emitted, live): emitted is a list of (done, issue, who, delta) in
    stream order (who NONE when there is no START entry, delta mod 2^64), live the rows whose
    entries are still in a map at the end, ascending."""
    who, issue, emitted = {}, {}, []
    for i in range(len(req)):
        if valid is not None and not valid[i]:
            continue
        r, k = int(req[i]), int(kind[i])
        if k == START:
            who[r] = i
        elif k == ISSUE:
            issue[r] = i
        elif k == DONE:
            if r not in issue:
                continue          # biotop.bpf.c:97-99: returns before whobyreq is touched
            j = issue.pop(r)
            w = who.pop(r, NONE)
            emitted.append((i, j, w, (int(ts[i]) - int(ts[j])) & U64))
    return emitted, sorted(list(who.values()) + list(issue.values()))


def join_arrays(req, kind, ts, valid=None):
    """join() as the arrays igx_req_join writes: done, issue, who (u32), delta (u64), live (u32)."""
    em, live = join(req, kind, ts, valid)
    cols = list(zip(*em)) if em else [(), (), (), ()]
    return (np.array(cols[0], np.uint32), np.array(cols[1], np.uint32), np.array(cols[2], np.uint32),
            np.array(cols[3], np.uint64), np.array(live, np.uint32))


def join_batches(req, kind, ts, cuts, valid=None):
    """The stream cut at `cuts` (ascending row numbers) and joined batch by batch, each batch
    with the live rows of the one before in front of it, in order (the in-band carry).  Returns
    (emitted, live) in global row numbers, comparable with join() over the whole stream."""
    n = len(req)
    bounds = [0] + list(cuts) + [n]
    carry = np.zeros(0, np.int64)          # global rows carried into the next batch
    emitted = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        rows = np.concatenate([carry, np.arange(a, b, dtype=np.int64)])
        v = None if valid is None else np.asarray(valid)[rows]
        em, live = join(np.asarray(req)[rows], np.asarray(kind)[rows], np.asarray(ts)[rows], v)
        for d, i, w, delta in em:
            emitted.append((int(rows[d]), int(rows[i]), NONE if w == NONE else int(rows[w]), delta))
        carry = rows[np.array(live, np.int64)] if live else np.zeros(0, np.int64)
    return emitted, [int(x) for x in carry]


def hand_cases():
    """The issue's ten hand cases: (name, req, kind, ts, emitted (done, issue, who), live rows)."""
    S, I, D = START, ISSUE, DONE
    a, b = 0xFFFF888800001000, 0xFFFF888800002000

    def case(name, kinds, emitted, live, reqs=None, ts=None):
        n = len(kinds)
        return (name, np.array(reqs if reqs is not None else [a] * n, np.uint64), np.array(kinds, np.uint8),
                np.array(ts if ts is not None else [1000 * (i + 1) for i in range(n)], np.uint64), emitted, live)

    return [
        case("S I D", [S, I, D], [(2, 1, 0)], []),
        case("I D D", [I, D, D], [(1, 0, NONE)], []),
        case("S D I D", [S, D, I, D], [(3, 2, 0)], []),
        case("S I S D", [S, I, S, D], [(3, 1, 2)], []),
        case("I I D", [I, I, D], [(2, 1, NONE)], []),
        case("S I D S", [S, I, D, S], [(2, 1, 0)], [3]),
        case("S I", [S, I], [], [0, 1]),
        case("D S", [D, S], [], [1]),
        case("Sa Ib Ia Db Da", [S, I, I, D, D], [(3, 1, NONE), (4, 2, 0)], [], reqs=[a, b, a, b, a]),
        case("I D(earlier ts) D", [I, D, D], [(1, 0, NONE)], [], ts=[5000, 4000, 6000]),
    ]


def random_stream(n, nreq, seed, p_kind=(0.3, 0.35, 0.35), wrap_ts=False):
    """n probe rows over nreq request pointers with the given START / ISSUE / DONE shares.
    wrap_ts: timestamps are not monotonic, so some deltas are negative as s64."""
    rng = np.random.default_rng(seed)
    pool = np.uint64(0xFFFF888000000000) + rng.choice(1 << 24, nreq, replace=False).astype(np.uint64) * np.uint64(256)
    req = pool[rng.integers(0, nreq, n)]
    kind = rng.choice(3, n, p=p_kind).astype(np.uint8)
    if wrap_ts:
        ts = rng.integers(0, 1 << 40, n).astype(np.uint64)
    else:
        ts = np.cumsum(rng.integers(1, 5000, n)).astype(np.uint64)
    return req, kind, ts
