"""tests/traceloop_ref.py (Tracer.Read's maps and loops restated row by row) pinned on hand-worked
groups.  Each case is a row list -- syscall rows (mono_ts, typ, id, pid[, sort_ts[, mntns]]) and
cont rows (mono_ts, index[, mntns]) -- with the events expected of it as (row, exit, class, conts).
tests/test_gpu_traceloop.py runs the same cases on the device (CASES is shared).  No GPU."""
import pytest

import traceloop_ref as R

NO = R.NO
E, X = 0, 1              # typ
EXIT_GROUP = 231
N6 = [NO] * 6


def conts(**kw):
    c = list(N6)
    for k, v in kw.items():
        c[int(k[1:])] = v
    return c


# (name, syscall rows, cont rows, expected events in output order)
CASES = [
    ("1 enter, exit, conts at indices 1 and 0",
     [(10, E, 1, 7), (10, X, 1, 7)], [(10, 1), (10, 0)], [(0, 1, 0, conts(i0=1, i1=0))]),
    ("2 two conts with the same index: the first row wins",
     [(10, E, 1, 7), (10, X, 1, 7)], [(10, 0), (10, 0)], [(0, 1, 0, conts(i0=0))]),
    ("3 an enter with no exit: incomplete, no parameters",
     [(10, E, 1, 7)], [(10, 0)], [(0, NO, 1, N6)]),
    ("4 an exit alone", [(10, X, 1, 7)], [], [(0, NO, 2, N6)]),
    ("5 conts alone", [], [(10, 0), (10, 1)], []),
    ("6 exit_group alone: complete, no exit row", [(10, E, EXIT_GROUP, 7)], [], [(0, NO, 0, N6)]),
    ("7 A matched, B would match too: only A",
     [(10, E, 1, 7), (10, E, 2, 8), (10, X, 1, 7), (10, X, 2, 8)], [], [(0, 2, 0, N6)]),
    ("8 A unmatched, B matched: only B, without the conts; A is dropped",
     [(10, E, 1, 7), (10, E, 2, 8), (10, X, 2, 8)], [(10, 0)], [(1, 2, 0, N6)]),
    ("9 A exit_group, B matched: both, A has the conts",
     [(10, E, EXIT_GROUP, 7), (10, E, 2, 8), (10, X, 2, 8)], [(10, 0)],
     [(0, NO, 0, conts(i0=0)), (1, 2, 0, N6)]),
    ("10 A exit_group and an unmatched exit: A complete, the exit incomplete",
     [(10, E, EXIT_GROUP, 7), (10, X, 3, 9)], [], [(0, NO, 0, N6), (1, NO, 2, N6)]),
    ("11 the only exit has the id but another pid: incomplete enter and incomplete exit",
     [(10, E, 1, 7), (10, X, 1, 8)], [], [(0, NO, 1, N6), (1, NO, 2, N6)]),
    ("12 a cont with index 6 is ignored",
     [(10, E, 1, 7), (10, X, 1, 7)], [(10, 6)], [(0, 1, 0, N6)]),
    ("13 the same mono_ts in two mount namespaces: two groups",
     [(10, E, 1, 7, 10, 1), (10, X, 1, 7, 10, 2)], [], [(0, NO, 1, N6), (1, NO, 2, N6)]),
    ("14 a typ 2 row does not exist",
     [(10, 2, 1, 7), (10, X, 1, 7)], [], [(1, NO, 2, N6)]),
    ("15 equal sort_ts: ordered by row",
     [(11, E, 1, 7, 5), (10, E, 1, 7, 5), (12, E, 1, 7, 4)], [], [(2, NO, 1, N6), (0, NO, 1, N6), (1, NO, 1, N6)]),
]


def columns(rows, crows):
    """The join's columns of a case; mntns columns only if a row names one."""
    with_mn = any(len(r) > 5 for r in rows) or any(len(c) > 2 for c in crows)
    col = dict(mono_ts=[r[0] for r in rows], typ=[r[1] for r in rows], id=[r[2] for r in rows],
               pid=[r[3] for r in rows], sort_ts=[r[4] if len(r) > 4 else r[0] for r in rows],
               c_mono_ts=[c[0] for c in crows], c_index=[c[1] for c in crows])
    if with_mn:
        col["mntns"] = [r[5] if len(r) > 5 else 1 for r in rows]
        col["c_mntns"] = [c[2] if len(c) > 2 else 1 for c in crows]
    return col


def events_of(out):
    row, ex, cls, cont = out
    return [(row[j], ex[j], cls[j], list(cont[6 * j:6 * j + 6])) for j in range(len(row))]


@pytest.mark.parametrize("case", CASES, ids=[c[0].split()[0] for c in CASES])
def test_hand_worked_group(case):
    _, rows, crows, want = case
    assert events_of(R.join(**columns(rows, crows))) == want


def test_valid_masks_and_arm64_numbers():
    # the exit row is masked out: the enter is incomplete; the masked cont is not taken
    col = columns([(10, E, 1, 7), (10, X, 1, 7)], [(10, 0), (10, 0)])
    assert events_of(R.join(**col, valid=[1, 0], c_valid=[0, 1])) == [(0, NO, 1, N6)]
    assert events_of(R.join(**col, c_valid=[0, 1])) == [(0, 1, 0, conts(i0=1))]
    # arm64: 94 is exit_group, 231 an ordinary number
    col = columns([(10, E, 94, 7), (11, E, 231, 7)], [])
    assert events_of(R.join(**col, nr=R.NR_ARM64)) == [(0, NO, 0, N6), (1, NO, 1, N6)]


def test_concatenated_cases_are_independent():
    """Every case at its own timestamp in one stream gives every case's events."""
    rows, crows, want = [], [], []
    for k, (_, r, c, w) in enumerate(CASES):
        base, rb, cb = 1000 * (k + 1), len(rows), len(crows)
        rows += [(base + x[0],) + tuple(x[1:4]) + (base + (x[4] if len(x) > 4 else x[0]),) + tuple(x[5:6] or (1,)) for x in r]
        crows += [(base + x[0], x[1]) + tuple(x[2:3] or (1,)) for x in c]
        want += [(e[0] + rb, e[1] if e[1] == NO else e[1] + rb, e[2], [v if v == NO else v + cb for v in e[3]]) for e in w]
    assert events_of(R.join(**columns(rows, crows))) == want
