"""Time igx_seccomp_update (advise seccomp-profile's per-mntns syscall sets) on one
GPU, in both mark forms, and state the host loop it replaces beside it.

The stream is synthetic and built on the device: ROWS sys_enter rows over MNTNS mount namespaces
drawn Zipf(1.1), syscall ids drawn Zipf(1.1) over IDS of the 500, and RUNC_SHARE of the rows from
runc, whose rows walk runc's start-up sequence (set-up calls, prctl(PR_GET_PDEATHSIG), the two
excluded calls, then the workload's first calls) in stream order.  comm is the tracer's 16-byte
column.

Timing: HIP events around the call after WARMUP calls on the same object, REPS times, median --
the map then already holds the stream's sets, as it does for all but the first seconds of a
trace; the first call on the empty map is stated beside it.  The LDS form runs at capacity 1024
(2048 slots, the reference's own max_entries), the global form at capacity 2^16.  The host figure
is the row-by-row restatement the tests compare against (tests/seccomp_ref.py) over the first
HOST_ROWS rows, whose result is also checked against the device's on a fresh object.  Prints one
JSON line (and writes it to --out).
    python tools/bench_seccomp.py [--out profiles/seccomp/bench_seccomp.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS = 100_000_000
MNTNS = 1024
IDS = 330
RUNC_SHARE = 0.01
WARMUP, REPS = 2, 10
HOST_ROWS = 1 << 20
HBM_BYTES_PER_S = 8e12
PRCTL, SECCOMP = 157, 317
# (id, arg0) of runc's rows, in order: clone, mount, chroot, prctl(2), prctl(38), seccomp, close, execve
STARTUP = [(56, 0), (165, 0), (161, 0), (PRCTL, 2), (PRCTL, 38), (SECCOMP, 1), (3, 0), (59, 0)]
FORMS = {"lds": 1024, "global": 1 << 16}


def zipf_draw(torch, n, k, s, g):
    w = torch.arange(1, k + 1, dtype=torch.float64, device="cuda") ** -s
    cdf = torch.cumsum(w / w.sum(), 0).to(torch.float32)
    u = torch.rand(n, generator=g, device="cuda")
    return torch.searchsorted(cdf, u).clamp_(max=k - 1)


def build_stream(torch, n):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EC)
    ns_pool = 4026531840 + torch.randperm(1 << 20, generator=g, device="cuda")[:MNTNS]
    id_pool = torch.randperm(500, generator=g, device="cuda")[:IDS]
    mntns = ns_pool[zipf_draw(torch, n, MNTNS, 1.1, g)]
    ids = id_pool[zipf_draw(torch, n, IDS, 1.1, g)].to(torch.int32)
    arg0 = torch.randint(0, 64, (n,), generator=g, device="cuda")
    runc = torch.rand(n, generator=g, device="cuda") < RUNC_SHARE
    step = (torch.cumsum(runc.to(torch.int64), 0) - 1) % len(STARTUP)       # the runc rows walk the sequence
    seq = torch.tensor(STARTUP, dtype=torch.int64, device="cuda")
    ids = torch.where(runc, seq[step, 0].to(torch.int32), ids)
    arg0 = torch.where(runc, seq[step, 1], arg0)
    comm = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
    comm[:, :5] = torch.tensor(list(b"nginx"), dtype=torch.uint8, device="cuda")
    comm[runc, :13] = torch.tensor(list(b"runc:[2:INIT]"), dtype=torch.uint8, device="cuda")
    compat = torch.zeros(n, dtype=torch.uint8, device="cuda")
    return ns_pool, (mntns.view(torch.uint64), ids.view(torch.uint32), arg0.view(torch.uint64), comm, compat)


def bytes_per_row(comm_stride, has_compat=True, has_valid=False):
    """Algorithmic HBM bytes per row.  The gate launch reads mntns (8), id (4), arg0 (8), compat and
    valid (1 each where given) and four bytes of comm -- but memory is fetched in 64-byte pieces,
    so of a comm column with a row stride up to 64 every byte is fetched: min(stride, 64) per
    row; it writes the u32 code (4).  The mark launch reads the code (4).  Slot, gate and bitmap
    traffic is per namespace, not per row, and is served from cache."""
    return 8 + 4 + 8 + min(comm_stride, 64) + int(has_compat) + int(has_valid) + 4 + 4


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--rows", type=int, default=ROWS)
    a = p.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_seccomp: needs a GPU")
    igx = importlib.import_module("inspektor-gadget_amd")
    from seccomp_ref import SeccompRef
    E, H = igx.engine, igx.columns
    n = a.rows
    ns_pool, cols = build_stream(torch, n)
    bpr = bytes_per_row(int(cols[3].stride(0)))
    forms = {}
    for form, capacity in FORMS.items():
        m = E.SeccompMap(capacity, PRCTL, SECCOMP)
        times = []
        for rep in range(1 + WARMUP + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.update(*cols)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        first, timed = times[0], sorted(times[1 + WARMUP:])
        med = timed[len(timed) // 2]
        forms[form] = {"capacity": capacity, "slots": m.slots(), "entries": m.count(),
                       "median_ms": round(med, 3), "min_ms": round(timed[0], 3), "max_ms": round(timed[-1], 3),
                       "first_call_ms": round(first, 3), "rows_per_s": round(n / (med * 1e-3)),
                       "fraction_of_8TBps": round(n * bpr / (med * 1e-3) / HBM_BYTES_PER_S, 4)}
        m.destroy()
    # the host loop over a sample, and the device on the same sample
    k = min(HOST_ROWS, n)
    h = [H.host(t[:k]) for t in cols]
    ref = SeccompRef(PRCTL, SECCOMP)
    t0 = time.perf_counter()
    ref.feed(*h)
    host_s = time.perf_counter() - t0
    keys = [int(x) for x in H.host(ns_pool)]
    same = True
    for capacity in FORMS.values():
        m = E.SeccompMap(capacity, PRCTL, SECCOMP)
        m.update(*(t[:k] for t in cols))
        val, found = m.peek(keys)
        for i, key in enumerate(keys):
            want = ref.lookup(key)
            same = same and bool(found[i]) == (want is not None) and val[i].tobytes() == (want or bytes(501))
        m.destroy()
    out = {"rows": n, "mntns": MNTNS, "ids": IDS, "runc_share": RUNC_SHARE, "reps": REPS, "forms": forms,
           "algorithmic_bytes_per_row": bpr, "ms_at_8TBps": round(n * bpr / HBM_BYTES_PER_S * 1e3, 3),
           "host_rows": k, "host_loop_s": round(host_s, 3), "host_rows_per_s": round(k / host_s),
           "sample_matches_restatement": bool(same), "device": torch.cuda.get_device_name(0),
           "note": "measured values, not targets"}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("bench_seccomp: the device map differs from the restatement on the sample")


if __name__ == "__main__":
    main()
