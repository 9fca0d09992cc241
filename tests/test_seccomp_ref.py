"""tests/seccomp_ref.py pinned on hand-written streams: one stream per rule of ig_seccomp_e
(seccomp.bpf.c:67-139), with the expected bytes written out by hand.  No GPU."""
from seccomp_ref import SeccompRef

PRCTL, SECCOMP = 157, 317
RUNC = b"runc:[2:INIT]\0\0\0"
SH = b"sh"


def value(ids=(), armed=0):
    v = bytearray(501)
    for i in ids:
        v[i] = 1
    v[500] = armed
    return bytes(v)


def test_dropped_rows_make_no_entry():
    r = SeccompRef()
    r.row(7, 1, 0, SH, compat=1)      # compat
    r.row(7, 500, 0, SH)              # id >= 500
    r.row(7, 0xFFFFFFFF, 0, SH)
    r.row(0, 1, 0, SH)                # mntns 0
    assert r.lookup(7) is None
    assert r.lookup(0) == value()     # the blank value at key 0 stays blank


def test_entry_exists_from_the_first_surviving_row():
    r = SeccompRef()
    r.row(7, 59, 0, RUNC)             # a runc row before the gate records nothing, but the entry is made
    assert r.lookup(7) == value()
    assert r.lookup(8) is None


def test_is_runc_is_the_first_four_bytes():
    r = SeccompRef()
    for m, comm in ((1, b"runc"), (2, RUNC), (3, b"run"), (4, b"runx"), (5, b"Runc"), (6, b"runcrunc" * 2)):
        r.row(m, 3, 0, comm)
    assert [r.lookup(m) for m in (1, 2, 6)] == [value()] * 3          # runc: held back
    assert [r.lookup(m) for m in (3, 4, 5)] == [value([3])] * 3       # not runc: recorded


def test_all_64_bits_of_arg0_are_compared():
    r = SeccompRef()
    r.row(7, PRCTL, 2 + (1 << 32), RUNC)     # not PR_GET_PDEATHSIG: does not arm
    r.row(7, 1, 0, RUNC)
    assert r.lookup(7) == value()
    r.row(7, PRCTL, 2, RUNC)                 # arms
    r.row(7, PRCTL, 38 + (1 << 32), RUNC)    # not PR_SET_NO_NEW_PRIVS: recorded as a prctl
    assert r.lookup(7) == value([PRCTL], 1)


def test_unarmed_runc_rows_record_nothing_and_prctl_2_arms():
    r = SeccompRef()
    r.row(7, 56, 0, RUNC)
    r.row(7, PRCTL, 38, RUNC)
    r.row(7, SECCOMP, 0, RUNC)
    assert r.lookup(7) == value()
    r.row(7, PRCTL, 2, RUNC)                 # arms, and is not itself recorded
    assert r.lookup(7) == value([], 1)


def test_armed_runc_rows_record_except_the_two_excluded_calls():
    r = SeccompRef()
    r.row(7, PRCTL, 2, RUNC)
    r.row(7, PRCTL, 38, RUNC)                # excluded
    r.row(7, SECCOMP, 1, RUNC)               # excluded
    assert r.lookup(7) == value([], 1)
    r.row(7, 59, 0, RUNC)
    assert r.lookup(7) == value([59], 1)
    r.row(7, PRCTL, 2, RUNC)                 # a later prctl(2) is recorded
    assert r.lookup(7) == value([59, PRCTL], 1)


def test_non_runc_rows_always_record():
    r = SeccompRef()
    r.row(7, 0, 0, SH)
    r.row(7, 499, 0, SH)
    r.row(7, PRCTL, 2, SH)                   # not runc: recorded, arms nothing
    r.row(7, SECCOMP, 0, SH)
    assert r.lookup(7) == value([0, 499, PRCTL, SECCOMP], 0)
    r.row(7, 12, 0, RUNC)                    # still unarmed
    assert r.lookup(7) == value([0, 499, PRCTL, SECCOMP], 0)


def test_gate_is_per_namespace():
    r = SeccompRef()
    r.row(1, PRCTL, 2, RUNC)
    r.row(2, 59, 0, RUNC)
    r.row(1, 59, 0, RUNC)
    assert r.lookup(1) == value([59], 1) and r.lookup(2) == value()


def test_delete_starts_from_blank():
    r = SeccompRef()
    r.row(7, PRCTL, 2, RUNC)
    r.row(7, 59, 0, RUNC)
    r.delete(7)
    assert r.lookup(7) is None
    r.row(7, 60, 0, RUNC)                    # the gate is gone too
    assert r.lookup(7) == value()
    r.delete(9)                              # never fed
    assert r.lookup(9) is None


def test_arm64_numbers_and_feed_mask():
    r = SeccompRef(167, 277)
    r.feed([7, 7, 7, 7], [157, 167, 277, 157], [2, 2, 0, 2], [RUNC] * 4, compat=None, valid=[1, 1, 1, 1])
    assert r.lookup(7) == value([157], 1)    # 157 is not prctl here; 167 arms; 277 is seccomp
    r = SeccompRef()
    r.feed([7, 7], [PRCTL, 59], [2, 0], [RUNC, RUNC], valid=[0, 1])
    assert r.lookup(7) == value()            # the arming row never reached the program
