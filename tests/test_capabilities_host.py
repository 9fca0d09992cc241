"""trace capabilities' host side (gadgets.py) without a GPU: the capability names, Audit / InsetID
on both sides of kernel 5.1.0, the verdict, the syscall name, the three column extractors and the
render; capsNames against the three cases of the reference's caps_name_test.go (kept as data in
tests/golden/capabilities_names.json); and the restatement tests/capabilities_ref.py on hand-made
probe sequences."""
import json
import os

import numpy as np

import capabilities_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capabilities_names.json")


def test_caps_names_golden(igx):
    G = igx.gadgets
    cases = json.load(open(GOLDEN))["cases"]
    assert sorted(cases) == ["all", "empty", "two_caps"]
    for name, c in cases.items():
        assert G.capsNames(int(c["bitfield"], 16)) == c["expected"], name


def test_capability_names(igx):
    G = igx.gadgets
    assert len(G.CAPABILITY_NAMES) == 41 and G.CAP_LAST_CAP == 40
    assert [G.capabilityName(i) for i in (0, 12, 21, 37, 38, 39, 40)] == \
        ["CHOWN", "NET_ADMIN", "SYS_ADMIN", "AUDIT_READ", "PERFMON", "BPF", "CHECKPOINT_RESTORE"]
    assert G.capabilityName(41) == "UNKNOWN (41)" and G.capabilityName(-1) == "UNKNOWN (-1)"
    assert all(n == n.upper() for n in G.CAPABILITY_NAMES)
    # bits 38..40 by the tracer's own table, nothing above 40
    assert G.capsNames(0xFFFFFFFFFFFFFFFF)[-3:] == ["perfmon", "bpf", "checkpoint_restore"]
    assert len(G.capsNames(0xFFFFFFFFFFFFFFFF)) == 41 and G.capsNames(1 << 41) == []


def _event(G, version, cap_opt, ret=0, syscall=-1, cap=21, caps=0x240000, names=None):
    return G.capabilities_event(G.kernelVersion(*version), {0: "read", 41: "socket"} if names is None else names,
                                pid=77, uid=1000, mntns=4026531840, comm=b"ping\0junk", ret=ret, ts=5000,
                                current_userns=4026531837, target_userns=4026531838, cap_effective=caps, cap=cap,
                                cap_opt=cap_opt, syscall=syscall, boot_to_wall_ns=7)


def test_kernel_version(igx):
    G = igx.gadgets
    assert G.kernelVersion(5, 1, 0) == 0x050100 and G.kernelVersion(4, 19, 300) == (4 << 16) + (19 << 8) + 255


def test_audit_and_insetid_by_kernel_version(igx):
    G = igx.gadgets
    for opt, audit, inset in ((0, 1, False), (2, 0, False), (4, 1, True), (6, 0, True), (1, 1, False)):
        for version in ((5, 1, 0), (6, 8, 0)):
            e = _event(G, version, opt)
            assert (e.Audit, e.InsetID) == (audit, inset), (opt, version)
    for opt in (0, 1, 2, 6):
        e = _event(G, (5, 0, 255), opt)
        assert (e.Audit, e.InsetID) == (opt, None)
        assert _event(G, (4, 19, 0), opt).Audit == opt


def test_event_fields(igx):
    G = igx.gadgets
    e = _event(G, (5, 15, 0), 0, ret=0, syscall=41)
    assert (e.Timestamp, e.MountNsID, e.Pid, e.Comm, e.Syscall, e.UID, e.Cap, e.CapName, e.Verdict) == \
        (5007, 4026531840, 77, "ping", "socket", 1000, 21, "SYS_ADMIN", "Allow")
    assert (e.TargetUserNs, e.CurrentUserNs, e.Caps, e.CapsNames) == (4026531838, 4026531837, 0x240000,
                                                                      ["sys_chroot", "sys_admin"])
    assert _event(G, (5, 15, 0), 0, ret=-1).Verdict == "Deny" and _event(G, (5, 15, 0), 0, ret=1).Verdict == "Deny"
    assert _event(G, (5, 15, 0), 0, syscall=0).Syscall == "read"          # syscall 0 is a syscall
    assert _event(G, (5, 15, 0), 0, syscall=-1).Syscall == ""             # no current_syscall entry
    assert _event(G, (5, 15, 0), 0, syscall=999).Syscall == ""            # a number without a name
    assert _event(G, (5, 15, 0), 0, syscall=(1 << 64) - 1).Syscall == ""  # ScmpSyscall is an int32
    assert _event(G, (5, 15, 0), 0, cap=63).CapName == "UNKNOWN (63)"


def test_extractors_and_render(igx):
    G = igx.gadgets
    cm = G.CapabilitiesColumns().cols
    new, old = _event(G, (5, 15, 0), 4, syscall=41), _event(G, (4, 19, 0), 1, ret=-1, caps=0)
    assert cm["insetid"].Extractor(new) == "true" and cm["insetid"].Extractor(_event(G, (5, 15, 0), 0)) == "false"
    assert cm["insetid"].Extractor(old) == "N/A"
    assert cm["caps"].Extractor(new) == "240000" and cm["caps"].Extractor(old) == "0"
    assert cm["capsnames"].Extractor(new) == "sys_chroot,sys_admin" and cm["capsnames"].Extractor(old) == ""
    assert [k for k, c in cm.items() if not c.Visible] == ["node", "namespace", "pod", "container", "timestamp", "mntns",
                                                           "insetid", "targetuserns", "currentuserns", "caps",
                                                           "capsnames"]
    assert (cm["cap"].Width, cm["cap"].FixedWidth, cm["capname"].Width, cm["verdict"].Width, cm["uid"].MinWidth) == \
        (3, True, 18, 7, 6)
    lines = G.capabilities_render([new, old]).split("\n")
    assert lines[0].split() == ["PID", "COMM", "SYSCALL", "UID", "CAP", "CAPNAME", "AUDIT", "VERDICT"]
    assert lines[1].split() == ["77", "ping", "socket", "1000", "21", "SYS_ADMIN", "1", "Allow"]
    assert lines[2].split() == ["77", "ping", "1000", "21", "SYS_ADMIN", "1", "Deny"]
    shown = G.capabilities_render([new], columns=["pid", "insetid", "caps", "capsnames"]).split("\n")
    assert shown[1].split() == ["77", "true", "240000", "sys_chroot,sys_admin"]


def _rows(seq):
    """seq of (kind, thread, extras) -> the batch columns, one mount namespace per thread parity."""
    n = len(seq)
    ev = {"kind": np.array([s[0] for s in seq], np.uint8),
          "pid_tgid": np.array([(100 << 32) | s[1] for s in seq], np.uint64),
          "mntns": np.array([4026531840 + s[1] % 2 for s in seq], np.uint64),
          "ts": np.arange(n, dtype=np.uint64) + np.uint64(1000), "nr": np.zeros(n, np.uint64),
          "cap": np.full(n, 21, np.int32), "cap_opt": np.zeros(n, np.int32), "cred_is_real": np.ones(n, np.uint8),
          "current_userns": np.full(n, 1, np.uint64), "target_userns": np.full(n, 2, np.uint64),
          "cap_effective": np.full(n, 3, np.uint64), "ret": np.zeros(n, np.int32), "uid": np.zeros(n, np.uint32),
          "comm": np.zeros((n, 16), np.uint8)}
    for i, s in enumerate(seq):
        for k, v in (s[2] if len(s) > 2 else {}).items():
            ev[k][i] = v
    return ev


def test_restatement_on_hand_sequences():
    E, X, S, Z = R.CAP_ENTER, R.CAP_EXIT, R.SYS_ENTER, R.SYS_EXIT
    # the syscall entry survives two reads; sys_exit clears it; an exit without an entry is missed
    ev = _rows([(S, 1, {"nr": 41}), (E, 1), (X, 1), (E, 1), (X, 1), (Z, 1), (E, 1), (X, 1), (X, 1)])
    out = R.Machine().feed(ev)
    assert [(e["timestamp"], e["syscall"]) for e in out] == [(1002, 41), (1004, 41), (1007, -1)]
    # nr 0 pending, and no entry at all: "read" against ""
    out = R.Machine().feed(_rows([(S, 1, {"nr": 0}), (E, 1), (X, 1), (E, 2), (X, 2)]))
    assert [e["syscall"] for e in out] == [0, -1]
    # a skipped sys_enter does nothing: it does not clear the entry before it
    out = R.Machine().feed(_rows([(S, 1, {"nr": 41}), (S, 1, {"nr": 231}), (E, 1), (X, 1)]))
    assert [e["syscall"] for e in out] == [41]
    out = R.Machine(goarch="arm64").feed(_rows([(S, 1, {"nr": 41}), (S, 1, {"nr": 231}), (E, 1), (X, 1)]))
    assert [e["syscall"] for e in out] == [231]
    # filters of the kprobe: credentials, NOAUDIT on both sides of 5.1.0, audit-only off, pids
    seq = [(E, 1, {"cred_is_real": 0}), (X, 1), (E, 1, {"cap_opt": 2}), (X, 1), (E, 1, {"cap_opt": 0}), (X, 1)]
    assert [e["timestamp"] for e in R.Machine().feed(_rows(seq))] == [1005]
    assert [e["timestamp"] for e in R.Machine(version=R.kernel_version(4, 19, 0)).feed(_rows(seq))] == [1003]
    assert [e["timestamp"] for e in R.Machine(audit_only=False).feed(_rows(seq))] == [1003, 1005]
    assert R.Machine(my_pid=100).feed(_rows(seq)) == [] and R.Machine(targ_pid=101).feed(_rows(seq)) == []
    assert len(R.Machine(targ_pid=100).feed(_rows(seq))) == 1
    # the mount namespace filter holds for the kprobe and sys_enter, not for the kretprobe and sys_exit
    seq = [(S, 1, {"nr": 2}), (S, 2, {"nr": 2}), (E, 1), (E, 2), (X, 1), (X, 2)]
    out = R.Machine(mntns_filter=[4026531840]).feed(_rows(seq))
    assert [(e["pid"], e["mntnsid"], e["syscall"]) for e in out] == [(100, 4026531840, 2)]
    # unique: the second (cap, mntns) never reaches `start`, so the pending first one is not overwritten
    seq = [(E, 1, {"cap_effective": 7}), (E, 1, {"cap_effective": 9}), (X, 1), (E, 1), (X, 1), (E, 3), (X, 3),
           (E, 2), (X, 2), (E, 1, {"cap": 12}), (X, 1)]
    out = R.Machine(unique=True).feed(_rows(seq))
    assert [(e["timestamp"], e["cap_effective"], e["cap"]) for e in out] == [(1002, 7, 21), (1008, 3, 21), (1010, 3, 12)]
    # state crosses feeds
    m = R.Machine()
    assert m.feed(_rows([(S, 1, {"nr": 41}), (E, 1)])) == []
    assert [e["syscall"] for e in m.feed(_rows([(X, 1)]))] == [41]


def test_restatement_to_event(igx):
    G = igx.gadgets
    out = R.Machine().feed(_rows([(R.SYS_ENTER, 1, {"nr": 41}), (R.CAP_ENTER, 1, {"cap_opt": 4}),
                                  (R.CAP_EXIT, 1, {"ret": -1, "uid": 5, "comm": np.frombuffer(b"ab" + b"\0" * 14, np.uint8)})]))
    d = R.to_event(out[0], R.kernel_version(5, 15, 0), G.CAPABILITY_NAMES, {41: "socket"}, boot_to_wall_ns=3)
    e = G.capabilities_event(G.kernelVersion(5, 15, 0), {41: "socket"}, 100, 5, 4026531841, b"ab" + b"\0" * 14, -1, 1002,
                             1, 2, 3, 21, 4, 41, 3)
    assert d == {k: getattr(e, k) for k in d} and d["InsetID"] is True and d["Verdict"] == "Deny"
