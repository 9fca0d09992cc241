"""Sequential restatement of the two-register last-writer join (include/igx.h, igx_lw_join): the
`start` and `current_syscall` maps of capable.bpf.c:40-85, keyed by the thread, walked row by
row with Python dicts.  A helper for the tests of the device join, not a test module."""
import numpy as np

SET_A, SET_B, CLEAR_B, TAKE_A = 0, 1, 2, 3
NONE = 0xFFFFFFFF


def join(key, kind, valid=None):
    """One batch.  Returns (emitted, live): emitted is a list of (take, a, b) in stream order (b
    NONE when B is empty), live the rows still held in a register at the end, ascending."""
    A, B, emitted = {}, {}, []
    for i in range(len(key)):
        if valid is not None and not valid[i]:
            continue
        r, k = int(key[i]), int(kind[i])
        if k == SET_A:
            A[r] = i                    # capable.bpf.c:147
        elif k == SET_B:
            B[r] = i                    # :237
        elif k == CLEAR_B:
            B.pop(r, None)              # :246
        elif k == TAKE_A:
            if r not in A:
                continue                # :162-164: missed entry
            emitted.append((i, A.pop(r), B.get(r, NONE)))   # :184-193: B is read, A deleted
    return emitted, sorted(list(A.values()) + list(B.values()))


def join_arrays(key, kind, valid=None):
    """join() as the arrays igx_lw_join writes: take, a, b, live (u32)."""
    em, live = join(key, kind, valid)
    cols = list(zip(*em)) if em else [(), (), ()]
    return (np.array(cols[0], np.uint32), np.array(cols[1], np.uint32), np.array(cols[2], np.uint32),
            np.array(live, np.uint32))


def join_batches(key, kind, cuts, valid=None, join_fn=None):
    """The stream cut at `cuts` (ascending row numbers) and joined batch by batch, each batch
    with the live rows of the one before in front of it, in order (the in-band carry).  join_fn
    (key, kind, valid) -> (emitted, live) is the join under test (default: join).  Returns
    (emitted, live) in global row numbers, comparable with join() over the whole stream."""
    join_fn = join if join_fn is None else join_fn
    n = len(key)
    bounds = [0] + list(cuts) + [n]
    carry = np.zeros(0, np.int64)          # global rows carried into the next batch
    emitted = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        rows = np.concatenate([carry, np.arange(a, b, dtype=np.int64)])
        v = None if valid is None else np.asarray(valid)[rows]
        em, live = join_fn(np.asarray(key)[rows], np.asarray(kind)[rows], v)
        for t, ra, rb in em:
            emitted.append((int(rows[t]), int(rows[ra]), NONE if rb == NONE else int(rows[rb])))
        carry = rows[np.array(live, np.int64)] if len(live) else np.zeros(0, np.int64)
    return emitted, [int(x) for x in carry]


def hand_cases():
    """(name, key, kind, emitted (take, a, b), live rows)."""
    A, B, C, T = SET_A, SET_B, CLEAR_B, TAKE_A
    x, y = 0x0000123400001234, 0x0000123400001235

    def case(name, kinds, emitted, live, keys=None):
        n = len(kinds)
        return (name, np.array(keys if keys is not None else [x] * n, np.uint64), np.array(kinds, np.uint8),
                emitted, live)

    return [
        case("A T", [A, T], [(1, 0, NONE)], []),
        case("B A T", [B, A, T], [(2, 1, 0)], [0]),
        case("B A T A T", [B, A, T, A, T], [(2, 1, 0), (4, 3, 0)], [0]),      # B survives reads
        case("B C A T", [B, C, A, T], [(3, 2, NONE)], []),
        case("T", [T], [], []),
        case("B T A", [B, T, A], [], [0, 2]),                                  # a TAKE on empty A keeps B
        case("A A T T", [A, A, T, T], [(2, 1, NONE)], []),
        case("A B B T", [A, B, B, T], [(3, 0, 2)], [2]),
        case("A T C", [A, T, C], [(1, 0, NONE)], []),
        case("C C", [C, C], [], []),
        case("Ax By Ay Tx Ty", [A, B, A, T, T], [(3, 0, NONE), (4, 2, 1)], [1], keys=[x, y, y, x, y]),
        case("A B", [A, B], [], [0, 1]),
        case("A B C", [A, B, C], [], [0]),
    ]


def random_stream(n, nkeys, seed, p_kind=(0.12, 0.38, 0.38, 0.12)):
    """n rows over nkeys thread ids with the given SET_A / SET_B / CLEAR_B / TAKE_A shares."""
    rng = np.random.default_rng(seed)
    pool = (rng.choice(1 << 22, nkeys, replace=False).astype(np.uint64) << np.uint64(32)) | \
        rng.integers(1, 1 << 22, nkeys).astype(np.uint64)
    key = pool[rng.integers(0, nkeys, n)]
    kind = rng.choice(4, n, p=p_kind).astype(np.uint8)
    return key, kind
