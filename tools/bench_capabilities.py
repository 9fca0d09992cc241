"""Time igx_lw_join (trace capabilities' two-register last-writer join) on one GPU,
and igx_req_join on as many rows and keys beside it.

The stream is synthetic and built on the device: N_SYS syscalls start STEP_NS apart, syscall i
belongs to thread i mod THREADS and lasts DUR_MIN..DUR_MAX ns, less than the THREADS x STEP_NS a
thread takes to come round again; it contributes a sys_enter row (SET_B) at its start and a
sys_exit row (CLEAR_B) at its end, and CAP_SHARE of the syscalls also a cap_capable entry / return
pair (SET_A, TAKE_A) at a third and a half of the way.  The rows are put in timestamp order, so
the threads interleave.  The key is pid_tgid: pid = tid / 4 + 1000, tid = 2000 + thread.

igx_req_join runs on the same keys in the same order with the kinds mapped SET_A -> ISSUE,
TAKE_A -> DONE, SET_B -> START and CLEAR_B -> a kind that does not exist for it, so both joins
sort the same keys and emit the same number of rows (req_join also writes a delta per emission).

Timing: HIP events around each call after WARMUP rounds, REPS rounds, the two joins alternating
within a round, median and spread of each; a call includes its one host read (the sort's digit
plan).  The device result on the first HOST_ROWS rows is checked against tests/lwjoin_ref.py.
Prints one JSON line (and writes it to --out).  --rounds 1 --no-check is the form a kernel trace
wraps.
    python tools/bench_capabilities.py [--out profiles/capabilities/bench_capabilities.json]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_SYS = 1 << 24
THREADS = 1 << 15
STEP_NS = 100
DUR_MIN, DUR_MAX = 1000, 3_000_000          # below THREADS x STEP_NS = 3 276 800
CAP_SHARE = 0.03
WARMUP, REPS = 2, 10
HOST_ROWS = 1 << 20


def build_stream(torch, n_sys, threads):
    g = torch.Generator(device="cuda")
    g.manual_seed(0xCA9)
    i = torch.arange(n_sys, dtype=torch.int64, device="cuda")
    t0 = i * STEP_NS
    dur = torch.randint(DUR_MIN, DUR_MAX, (n_sys,), generator=g, device="cuda")
    has_cap = torch.rand(n_sys, generator=g, device="cuda") < CAP_SHARE
    ci = i[has_cap]
    # sections in lw kind order: SET_A (cap enter), SET_B (sys_enter), CLEAR_B (sys_exit), TAKE_A (cap exit)
    ts = torch.cat([t0[ci] + dur[ci] // 3, t0, t0 + dur, t0[ci] + dur[ci] // 2])
    sysno = torch.cat([ci, i, i, ci])
    kind = torch.cat([torch.full((ci.numel(),), 0, dtype=torch.uint8, device="cuda"),
                      torch.full((n_sys,), 1, dtype=torch.uint8, device="cuda"),
                      torch.full((n_sys,), 2, dtype=torch.uint8, device="cuda"),
                      torch.full((ci.numel(),), 3, dtype=torch.uint8, device="cuda")])
    del t0, dur, has_cap, i
    ts, order = torch.sort(ts, stable=True)
    kind, thread = kind[order], sysno[order] % threads
    del order, sysno
    key = ((thread // 4 + 1000) << 32) | (thread + 2000)
    return key.view(torch.uint64), kind, ts.view(torch.uint64)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--syscalls", type=int, default=N_SYS)
    p.add_argument("--threads", type=int, default=THREADS)
    p.add_argument("--rounds", type=int, default=REPS)
    p.add_argument("--no-check", action="store_true")
    a = p.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_capabilities: needs a GPU")
    igx = importlib.import_module("inspektor-gadget_amd")
    import lwjoin_ref as R
    E, H, A = igx.engine, igx.columns, igx._abi
    key, kind, ts = build_stream(torch, a.syscalls, a.threads)
    n = int(key.numel())
    to_req = torch.tensor([A.REQ_ISSUE, A.REQ_START, 3, A.REQ_DONE], dtype=torch.uint8, device="cuda")
    rkind = to_req[kind.to(torch.int64)]
    t_lw, t_rj = [], []
    warm = min(WARMUP, a.rounds - 1)
    for rep in range(warm + a.rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        j = E.lw_join(key, kind, sync=False)
        ev[1].record()
        ev[2].record()
        r = E.req_join(key, rkind, ts, sync=False)
        ev[3].record()
        torch.cuda.synchronize()
        if rep >= warm:
            t_lw.append(ev[0].elapsed_time(ev[1]))
            t_rj.append(ev[2].elapsed_time(ev[3]))
        nt, npend = int(j["n_take"].cpu().view(torch.int64)), int(j["n_pend"].cpu().view(torch.int64))
        nd = int(r["n_done"].cpu().view(torch.int64))
        del j, r
    t_lw.sort()
    t_rj.sort()
    med_lw, med_rj = t_lw[len(t_lw) // 2], t_rj[len(t_rj) // 2]
    same = None
    if not a.no_check:
        m = min(HOST_ROWS, n)
        take, ra, rb, live = R.join_arrays(H.host(key[:m]), H.host(kind[:m]))
        js = E.lw_join(key[:m], kind[:m])
        same = all(np.array_equal(H.host(js[k]).view(np.uint32), w) for k, w in
                   (("take", take), ("a", ra), ("b", rb), ("pend", live)))
    out = {"rows": n, "syscalls": a.syscalls, "threads": a.threads, "cap_share": CAP_SHARE, "n_take": nt, "n_pend": npend,
           "req_join_n_done": nd, "rounds": a.rounds,
           "lw_join_median_ms": round(med_lw, 3), "lw_join_min_ms": round(t_lw[0], 3), "lw_join_max_ms": round(t_lw[-1], 3),
           "req_join_median_ms": round(med_rj, 3), "req_join_min_ms": round(t_rj[0], 3),
           "req_join_max_ms": round(t_rj[-1], 3), "lw_over_req": round(med_lw / med_rj, 4),
           "lw_join_rows_per_s": round(n / (med_lw * 1e-3)), "sample_matches_restatement": same,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if same is False:
        raise SystemExit("bench_capabilities: the device join differs from the restatement on the sample")


if __name__ == "__main__":
    main()
