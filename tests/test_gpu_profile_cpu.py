"""gadgets.ProfileCpuTracer on the device against the probe + collectResult restated over
Python values (tests/stack_ref.py): about 50 000 samples over a few hundred stacks at depth 127,
with tid 0 rows, failed stack walks of two kinds, user addresses in ip and equal counts, in one
feed and in three, for every option combination; and profile/cpu through the registry."""
import json

import numpy as np
import pytest

from stack_ref import ProfileCpuRef

pytestmark = pytest.mark.gpu

DEPTH = 127
KBASE = 0xffffffff81000000
COLS = ("pid", "tid", "mntns", "comm", "ip", "kstack", "kstatus", "ustack", "ustatus")


@pytest.fixture(scope="module")
def workload():
    rng = np.random.default_rng(21)
    n, nk, nu = 50021, 300, 200
    # A table that starts out of order: a frame below the second symbol ends the search at
    # symbol 0 with a lower address probed last, the one way to "[unknown]" (tracer.go:203).
    syms = [(KBASE + 0x400 * 5000, "misplaced")] + [(KBASE + 0x400 * i, f"ksym_{i}") for i in range(1, 2000)]
    # modules after the core symbols, not in address order
    syms += [(KBASE + 0x400 * (2000 + int(i)), f"mod_{int(i)}") for i in rng.permutation(300)]

    def stacks(k, lo, hi):
        st = np.zeros((k, DEPTH), np.uint64)
        for r in range(k):
            d = DEPTH if r < 3 else int(rng.integers(1, DEPTH + 1))     # full-depth stacks too
            st[r, :d] = rng.integers(lo, hi, d, dtype=np.uint64)
        return st

    kpool = stacks(nk, KBASE - 0x1000, KBASE + 0x400 * 2310)
    upool = stacks(nu, 0x400000, 0x7fff00000000)
    procs = [(100 + p, 4026531840 + p % 5, f"proc-{p % 17}".encode().ljust(16, b"\0")) for p in range(40)]
    # a sample comes from one of 600 call sites (process, kernel stack, user stack), Zipf over them
    sites = np.stack([rng.integers(0, len(procs), 600), rng.integers(0, nk, 600), rng.integers(0, nu, 600)], 1)
    pr, ki, ui = sites[np.minimum(rng.zipf(1.2, n) - 1, 599)].T
    c = {"pid": np.array([procs[p][0] for p in pr], np.uint32),
         "tid": np.array([procs[p][0] + 1 for p in pr], np.uint32),
         "mntns": np.array([procs[p][1] for p in pr], np.uint64),
         "comm": np.array([np.frombuffer(procs[p][2], np.uint8) for p in pr]),
         "kstack": kpool[ki], "ustack": upool[ui],
         "kstatus": rng.integers(0, 1000, n).astype(np.int32), "ustatus": rng.integers(0, 1000, n).astype(np.int32)}
    # ip: the kernel stack's first frame, or a user address
    c["ip"] = np.where(rng.integers(0, 4, n) > 0, c["kstack"][:, 0], c["ustack"][:, 0]).astype(np.uint64)
    c["tid"][rng.integers(0, n, 700)] = 0                         # idle samples
    c["tid"][0] = 0                                               # the first one too
    c["kstatus"][rng.integers(0, n, 900)] = -14                   # -EFAULT
    c["kstatus"][rng.integers(0, n, 400)] = -17                   # -EEXIST
    c["ustatus"][rng.integers(0, n, 900)] = -14
    c["ustatus"][rng.integers(0, n, 400)] = -17
    # equal counts: a run of keys seen exactly twice each, far apart
    for j in range(30):
        for at in (1000 + j, 30000 - 7 * j):
            c["pid"][at], c["tid"][at], c["mntns"][at] = 9000 + j, 9000 + j, 77
            c["kstatus"][at] = c["ustatus"][at] = 0
            c["kstack"][at], c["ustack"][at] = kpool[j], upool[j]
            c["ip"][at] = kpool[j][0]
    return c, syms


def _host_cols(c, lo, hi):
    return [c["pid"][lo:hi].tolist(), c["tid"][lo:hi].tolist(), c["mntns"][lo:hi].tolist(),
            [r.tobytes() for r in c["comm"][lo:hi]], c["ip"][lo:hi].tolist(),
            [r.tobytes() for r in c["kstack"][lo:hi]], c["kstatus"][lo:hi].tolist(),
            [r.tobytes() for r in c["ustack"][lo:hi]], c["ustatus"][lo:hi].tolist()]


@pytest.fixture(scope="module")
def device_cols(igx, workload):
    c, _ = workload
    return {k: igx.columns.to_device(c[k]) for k in COLS}


OPTIONS = [dict(user_stack_only=u, kernel_stack_only=k, include_idle=i)
           for u in (False, True) for k in (False, True) for i in (False, True)]


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "".join("UKI"[j] if v else "-" for j, v in enumerate(o.values())))
def test_reports_equal_restatement(igx, workload, device_cols, opt):
    c, syms = workload
    n = len(c["pid"])
    ref = ProfileCpuRef(kallsyms=syms, **opt)
    ref.feed(*_host_cols(c, 0, n))
    want = ref.reports()
    want_json = ref.stop()
    assert len(want) > 50 and any(r["Count"] == want[i + 1]["Count"] for i, r in enumerate(want[:-1]))
    for cuts in ([0, n], [0, 17000, 17001, n]):
        tr = igx.gadgets.ProfileCpuTracer(depth=DEPTH, max_stacks=1024, capacity=1 << 16, kallsyms=syms, **opt)
        try:
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                tr.feed(**{k: device_cols[k][lo:hi] for k in COLS})
            got = tr.reports()
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert (g.Comm, g.Pid, g.UserStack, g.KernelStack, g.Count, g.MntnsID) == \
                    (w["Comm"], w["Pid"], w["UserStack"], w["KernelStack"], w["Count"], w["MntnsID"])
            assert tr.Stop() == want_json
            assert got[-1].ExtraLines() == ["\t" + s for s in reversed(want[-1]["KernelStack"])] + \
                ["\t" + s for s in reversed(want[-1]["UserStack"])]
        finally:
            tr.destroy()


def test_kallsyms_text_and_feeds_of_the_restatement(igx, workload, device_cols):
    """kallsyms given as the text of /proc/kallsyms, and the restatement fed in three parts too
    (its ids do not depend on the split either)."""
    c, syms = workload
    n = 6000
    text = "".join(f"{a:016x} t {name}\n" for a, name in syms) + "bad line\n"
    ref = ProfileCpuRef(kallsyms=syms)
    for lo, hi in ((0, 1), (1, 4097), (4097, n)):
        ref.feed(*_host_cols(c, lo, hi))
    tr = igx.gadgets.ProfileCpuTracer(depth=DEPTH, max_stacks=1024, capacity=1 << 12, kallsyms=text)
    try:
        tr.feed(**{k: device_cols[k][:n] for k in COLS})
        assert tr.Stop() == ref.stop()
    finally:
        tr.destroy()
    with pytest.raises(ValueError):
        igx.gadgets.ProfileCpuTracer(depth=DEPTH, max_stacks=16, capacity=16, kallsyms="0xzz t broken\n")


def test_profile_cpu_through_runtime(igx, workload, device_cols):
    OPS = igx.operators
    c, syms = workload
    desc = OPS.Get("profile", "cpu")
    assert desc is not None and desc.Type() == OPS.TypeProfile
    assert desc.Description() == "Analyze CPU performance by sampling stack traces"
    assert desc.ParamDescs() == {"user-stack": False, "kernel-stack": False}
    assert isinstance(desc.EventPrototype(), igx.gadgets.CpuReport)
    n = 5000
    batches = [{k: device_cols[k][lo:hi] for k in COLS} for lo, hi in ((0, 2000), (2000, n))]
    params = {"kernel-stack": True, "kallsyms": syms, "depth": DEPTH, "max-stacks": 1024, "capacity": 4096,
              "events": lambda i: batches if i == 0 else None}
    res = OPS.LocalRuntime().RunGadget(OPS.GadgetContext("t", desc, params))
    ref = ProfileCpuRef(kernel_stack_only=True, kallsyms=syms)
    ref.feed(*_host_cols(c, 0, n))
    assert res[""].decode() == ref.stop()
    assert json.loads(res[""])[-1]["count"] == ref.reports()[-1]["Count"]
