"""Time igx_req_join (the block-I/O start / issue / done pairing) on one GPU and
state the host loop it replaces beside it.

The stream is synthetic and built on the device: N_REQ requests arrive STEP_NS apart, request i
uses pointer POOL_BASE + (i mod POOL) * POOL_STRIDE (a recycled pool, as the block layer's
request cache), and contributes a START row at its arrival, an ISSUE row ISSUE_MIN..ISSUE_MAX ns
later and a DONE row LAT_MIN..LAT_MAX ns after that; the 3 x N_REQ rows are put in timestamp
order, so the three kinds interleave as completions trail arrivals.  LAT_MAX is below the time a
pointer takes to come round again (POOL x STEP_NS).

Timing: HIP events around the call after WARMUP calls, REPS times, median; the call includes its
one host read (the sort's digit plan).  The host figure is the Python / numpy restatement the
tests compare against (tests/reqjoin_ref.py) over the first HOST_ROWS rows, whose result is also
checked against the device's.  Prints one JSON line (and writes it to --out).
    python tools/bench_reqjoin.py [--out profiles/reqjoin/bench_reqjoin.json]
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

N_REQ = 1 << 25
POOL = 10240
POOL_BASE = 0xFFFF8881_0A400000
POOL_STRIDE = 320            # bytes between two requests of the pool
STEP_NS = 1000
ISSUE_MIN, ISSUE_MAX = 200, 2200
LAT_MIN, LAT_MAX = 20_000, 8_000_000
WARMUP, REPS = 2, 10
HOST_ROWS = 1 << 20
HBM_BYTES_PER_S = 8e12


def build_stream(torch, n_req):
    g = torch.Generator(device="cuda")
    g.manual_seed(0xB10)
    i = torch.arange(n_req, dtype=torch.int64, device="cuda")
    t_s = i * STEP_NS
    t_i = t_s + torch.randint(ISSUE_MIN, ISSUE_MAX, (n_req,), generator=g, device="cuda")
    t_d = t_i + torch.randint(LAT_MIN, LAT_MAX, (n_req,), generator=g, device="cuda")
    ts = torch.cat([t_s, t_i, t_d])
    del t_s, t_i, t_d
    ts, order = torch.sort(ts, stable=True)
    kind = (order // n_req).to(torch.uint8)
    req = (order % n_req % POOL) * POOL_STRIDE + (POOL_BASE - (1 << 64))      # the u64 pointer's bits as int64
    del order, i
    return req.view(torch.uint64), kind, ts.view(torch.uint64)


def bytes_per_row(done_share, live_digits):
    """Algorithmic HBM bytes per probe row, by pass (DESIGN.md §4 has the derivation)."""
    sort = 8 + 12 + live_digits * (4 + 8 + 8)      # compose; per live digit: histogram read, scatter read + write
    code = 4 + 8 + 1 + 1                           # perm, req, kind read; code written
    scan = 1 + (1 + 4)                             # summary reads code; apply reads code and perm
    flags = 1 + 1 + 1                              # cleared, counted, compacted
    per_done = (1 + 4 + 4 + 8) + (4 + 4 + 8 + 8) + (4 + 4 + 4 + 8)   # apply's writes and gathers; compaction in / out
    return sort + code + scan + flags + done_share * per_done


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--requests", type=int, default=N_REQ)
    a = p.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_reqjoin: needs a GPU")
    igx = importlib.import_module("inspektor-gadget_amd")
    import reqjoin_ref as R
    E, H = igx.engine, igx.columns
    req, kind, ts = build_stream(torch, a.requests)
    n = int(req.numel())
    times = []
    for rep in range(WARMUP + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        j = E.req_join(req, kind, ts, sync=False)
        e1.record()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            times.append(e0.elapsed_time(e1))
        nd, npend = int(j["n_done"].cpu().view(torch.int64)), int(j["n_pend"].cpu().view(torch.int64))
        del j
    times.sort()
    med = times[len(times) // 2]
    pool = POOL_BASE + np.arange(POOL, dtype=np.uint64) * np.uint64(POOL_STRIDE)
    diff = int(np.bitwise_or.reduce(pool)) ^ int(np.bitwise_and.reduce(pool))
    digits = sum(1 for b in range(8) if (diff >> (8 * b)) & 0xFF)
    bpr = bytes_per_row(nd / n, digits)
    # the host loop over a sample, and the device on the same sample
    m = min(HOST_ROWS, n)
    h = [H.host(t[:m]) for t in (req, kind, ts)]
    t0 = time.perf_counter()
    done, issue, who, delta, live = R.join_arrays(*h)
    host_s = time.perf_counter() - t0
    js = E.req_join(req[:m], kind[:m], ts[:m])
    same = all(np.array_equal(H.host(js[k]).view(np.uint32), w) for k, w in
               (("done", done), ("issue", issue), ("who", who), ("pend", live))) and \
        np.array_equal(H.host(js["delta"]), delta)
    out = {"rows": n, "requests": a.requests, "pool": POOL, "n_done": nd, "n_pend": npend,
           "median_ms": round(med, 3), "min_ms": round(times[0], 3), "max_ms": round(times[-1], 3), "reps": REPS,
           "rows_per_s": round(n / (med * 1e-3)), "live_sort_digits": digits,
           "algorithmic_bytes_per_row": round(bpr, 1), "ms_at_8TBps": round(n * bpr / HBM_BYTES_PER_S * 1e3, 3),
           "host_rows": m, "host_loop_s": round(host_s, 3), "host_rows_per_s": round(m / host_s),
           "sample_matches_restatement": bool(same), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("bench_reqjoin: the device join differs from the restatement on the sample")


if __name__ == "__main__":
    main()
