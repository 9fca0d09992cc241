"""Time igx_intern_add and igx_ksym_lookup (profile cpu on the device, DESIGN.md §4 k_stack) on
one GPU.

Steps, each run as a child process of its own under `timeout` (one at a time; the first that
fails ends the run):
  zipf      2M rows of 1016 bytes (a depth-127 stack), Zipf 1.1 over 64k distinct stacks
  distinct  2M rows of 1016 bytes, all distinct
  ksym      8M addresses against 200k sorted symbols
For the interner two figures per workload: `fresh`, the batch added to an empty interner (every
content is new once, and the distinct rows are appended to the store), and `resident`, the same
batch added again (every row is found in the store).  Timing: HIP events around the call after
WARMUP calls, REPS times, median.  The algorithmic bytes of an add are each input row read once
plus 4 bytes of ids; bytes_per_s is that over the median, stated against 8 TB/s.  The first and
last ids are checked against what the stream's construction implies.  Prints one JSON line per
step (and appends them to --out).
    python tools/bench_stack_intern.py [--out profiles/stack/bench_stack_intern.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ROWS = 1 << 21
DEPTH = 127
ROW_BYTES = DEPTH * 8
N_STACKS = 1 << 16
ZIPF_S = 1.1
N_IPS, N_SYMS = 1 << 23, 200_000
WARMUP, REPS = 2, 5
HBM_BYTES_PER_S = 8e12
STEPS = {"zipf": 420, "distinct": 420, "ksym": 240}    # seconds allowed per step


def _median_ms(torch, fn):
    times = []
    for rep in range(WARMUP + REPS):
        pre = fn(None)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(pre)
        e1.record()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def step_intern(torch, igx, name):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x57AC)
    if name == "zipf":
        pool = torch.randint(1, 1 << 62, (N_STACKS, DEPTH), generator=g, device="cuda", dtype=torch.int64)
        k = torch.arange(1, N_STACKS + 1, dtype=torch.float64, device="cuda")
        cdf = torch.cumsum(k ** (-ZIPF_S), 0)
        cdf /= cdf[-1].clone()
        pick = torch.searchsorted(cdf, torch.rand(N_ROWS, generator=g, device="cuda", dtype=torch.float64))
        pick.clamp_(max=N_STACKS - 1)
        rows = pool[pick]
        # ids by first appearance: the rank of each stack's first row among all first rows
        first = torch.full((N_STACKS,), N_ROWS, dtype=torch.int64, device="cuda")
        first.scatter_reduce_(0, pick, torch.arange(N_ROWS, device="cuda"), "amin")
        seen = first < N_ROWS
        rank = torch.empty(N_STACKS, dtype=torch.int64, device="cuda")
        order = torch.argsort(first)
        rank[order] = torch.arange(N_STACKS, device="cuda")
        want, distinct = rank[pick], int(seen.sum())
        del pool, cdf, k, first, order, rank
        cap = N_STACKS
    else:
        rows = torch.randint(1, 1 << 62, (N_ROWS, DEPTH), generator=g, device="cuda", dtype=torch.int64)
        rows[:, 0] = torch.arange(N_ROWS, device="cuda")
        want, distinct, cap = torch.arange(N_ROWS, device="cuda"), N_ROWS, N_ROWS
    rows8 = rows.view(torch.uint8)
    state = {}

    def fresh(pre):
        if pre is None:
            if state.get("t") is not None:
                state["t"].destroy()
            state["t"] = igx.engine.Interner(ROW_BYTES, cap)
            return True
        state["ids"] = state["t"].add(rows8)

    def resident(pre):
        if pre is None:
            return True
        state["ids"] = state["t"].add(rows8)

    out = {"step": name, "rows": N_ROWS, "row_bytes": ROW_BYTES, "distinct": distinct, "reps": REPS}
    bytes_alg = N_ROWS * (ROW_BYTES + 4)
    for label, fn in (("fresh", fresh), ("resident", resident)):
        med, lo, hi = _median_ms(torch, fn)
        ok = bool((state["ids"].to(torch.int64) == want).all()) and state["t"].count() == distinct
        out[label] = {"median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                      "rows_per_s": round(N_ROWS / (med * 1e-3)),
                      "bytes_per_s": round(bytes_alg / (med * 1e-3)),
                      "share_of_8TBps": round(bytes_alg / (med * 1e-3) / HBM_BYTES_PER_S, 4), "ids_match": ok}
    state["t"].destroy()
    out["algorithmic_bytes"] = bytes_alg
    return out, all(out[k]["ids_match"] for k in ("fresh", "resident"))


def step_ksym(torch, igx):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x515)
    base = 0xffffffff81000000 - (1 << 64)
    sym = (base + torch.cumsum(torch.randint(16, 4096, (N_SYMS,), generator=g, device="cuda"), 0)).view(torch.uint64)
    span = int(sym.view(torch.int64)[-1]) - base
    ips = (base + torch.randint(0, span + 4096, (N_IPS,), generator=g, device="cuda")).view(torch.uint64)
    state = {}

    def run(pre):
        if pre is None:
            return True
        state["idx"] = igx.engine.ksym_lookup(sym, ips)

    med, lo, hi = _median_ms(torch, run)
    # on a sorted table of distinct addresses the search is "last symbol <= ip" (symbol 0 below all)
    want = (torch.searchsorted(sym.view(torch.int64), ips.view(torch.int64), right=True) - 1).clamp_(min=0)
    ok = bool((state["idx"].to(torch.int64) == want).all())
    return {"step": "ksym", "addresses": N_IPS, "symbols": N_SYMS, "reps": REPS, "median_ms": round(med, 3),
            "min_ms": round(lo, 3), "max_ms": round(hi, 3), "lookups_per_s": round(N_IPS / (med * 1e-3)),
            "matches_searchsorted": ok}, ok


def run_step(name):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stack_intern: needs a GPU")
    igx = importlib.import_module("inspektor-gadget_amd")
    out, ok = step_ksym(torch, igx) if name == "ksym" else step_intern(torch, igx, name)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    if not ok:
        raise SystemExit(f"bench_stack_intern: step {name} differs from what the stream implies")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--step", choices=sorted(STEPS), default=None)
    a = p.parse_args()
    if a.step:
        return run_step(a.step)
    lines = []
    for name, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            raise SystemExit(f"bench_stack_intern: step {name} ended with status {r.returncode}; stopping")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
