"""Time igx_traceloop_join (traceloop's enter / exit / cont join) on one GPU, with
igx_req_join on as many rows beside it as a yardstick.

The stream is synthetic, seeded and built on the device: ROWS syscall rows over MNTNS containers,
as enter / exit pairs that share a monotonic timestamp of their own, a pid and an id; EXIT_SHARE of
the syscalls are exit_group (no exit row); CONT_SHARE of the syscalls carry one cont (parameter 0
or 1); COLLIDE of the syscalls take the timestamp and container of the syscall before them (two
CPUs stamping the same nanosecond); LOST of the rows are masked out (overwritten in the ring), which
leaves incomplete enters and exits.  Rows arrive in time order with local disorder (several rings
read one after another).  sort_ts is the boot timestamp.

Timing: HIP events around each call, WARMUP calls first, then REPS calls of the traceloop join
alternating with REPS calls of igx_req_join over ns + nc rows (the number the traceloop join's
first sort handles; its key is the same timestamps, its kinds are random) -- medians.  The
algorithmic bytes are those of the join's own passes (bytes_per_call); the two sorts are not
counted, since how many digit passes they run is decided from the data.  So the stated share of
HBM peak -- those bytes over the time of the whole call -- is a lower bound on the traffic.  The
first SAMPLE rows are also joined on the device and compared with the row-by-row restatement
(tests/traceloop_ref.py).  Prints one JSON line (and writes it to --out).
    python tools/bench_traceloop.py [--out profiles/traceloop/bench_traceloop.json]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS = 32_000_000
MNTNS = 1000
EXIT_SHARE, CONT_SHARE, COLLIDE, LOST = 0.002, 0.15, 0.01, 0.01
WARMUP, REPS = 2, 7
SAMPLE = 200_000
HBM_BYTES_PER_S = 8e12
NR = (60, 231, 15)


def build_stream(torch, ns):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x7AC)
    dev = "cuda"
    npair = ns // 2
    pool = 4026531840 + torch.randperm(1 << 20, generator=g, device=dev)[:MNTNS]
    ts = 10**12 + torch.arange(npair, device=dev, dtype=torch.int64) * 137 + torch.randint(0, 100, (npair,), generator=g, device=dev)
    mn = pool[torch.randint(0, MNTNS, (npair,), generator=g, device=dev)]
    hit = torch.rand(npair, generator=g, device=dev) < COLLIDE
    hit[0] = False
    # a run of hits all take the timestamp of the syscall before the run
    idx = torch.arange(npair, device=dev)
    src = torch.where(hit, torch.zeros_like(idx), idx)
    src = torch.cummax(src, 0).values
    ts, mn = ts[src], mn[src]
    groups = int(npair - hit.sum())
    pid = torch.randint(1, 5000, (npair,), generator=g, device=dev, dtype=torch.int32)
    sid = torch.randint(0, 330, (npair,), generator=g, device=dev, dtype=torch.int32)
    sid = torch.where(torch.rand(npair, generator=g, device=dev) < EXIT_SHARE, torch.full_like(sid, NR[1]), sid)
    sid = torch.where((sid == NR[0]) | (sid == NR[2]), torch.full_like(sid, 1), sid)
    rep = lambda t: t.repeat_interleave(2)   # noqa: E731
    typ = torch.arange(2 * npair, device=dev) % 2
    valid = torch.rand(2 * npair, generator=g, device=dev) >= LOST
    valid &= ~((typ == 1) & (rep(sid) == NR[1]))              # exit_group has no exit row
    order = torch.argsort(torch.arange(2 * npair, device=dev) + torch.randint(0, 64, (2 * npair,), generator=g, device=dev))
    cols = dict(mntns=rep(mn)[order].contiguous().view(torch.uint64), mono_ts=rep(ts)[order].contiguous().view(torch.uint64),
                typ=typ[order].to(torch.uint8), id=rep(sid)[order].to(torch.int16), pid=rep(pid)[order].contiguous(),
                valid=valid[order].to(torch.uint8))
    cols["sort_ts"] = (rep(ts)[order] + 5_000_000_000).view(torch.uint64)
    pick = torch.nonzero(torch.rand(npair, generator=g, device=dev) < CONT_SHARE).flatten()
    cols["c_mntns"] = mn[pick].contiguous().view(torch.uint64)
    cols["c_mono_ts"] = ts[pick].contiguous().view(torch.uint64)
    cols["c_index"] = torch.randint(0, 2, (len(pick),), generator=g, device=dev).to(torch.uint8)
    return cols, groups


def bytes_per_call(ns, nc, groups, nev, cont_groups, has_mntns=True, has_valid=True):
    """Algorithmic HBM bytes of the join's own passes (the two sorts excluded), n = ns + nc:
      pack     reads a syscall row's mntns 8, mono_ts 8, typ 1, id 2, pid 4, valid 1 and a cont row's
               mntns 8, mono_ts 8, index 1; writes three u64 keys per row (24)
      code     per position: the order 4, the row's three keys 24 (the neighbour's come from
               cache); writes the code 1
      summary  per position: code 1, order 4
      groups   per position: code 1, order 4; per group 16 written (+ 24 with conts)
      class    per position: code 1; per syscall row: order 4; per group 16 read; per event 6 written;
               the class and no-event bytes are preset, 2 per syscall row
      emit     per event: its row 4, class 1, group number 4, group result 16 (+ 24 with conts);
               per syscall row 33 written (ev_row, ev_exit, ev_class, ev_cont)"""
    n = ns + nc
    mn = 8 if has_mntns else 0
    pack = ns * (mn + 8 + 1 + 2 + 4 + int(has_valid)) + nc * (mn + 8 + 1) + n * (16 + mn)
    code = n * (4 + 16 + mn + 1)
    summary = n * 5
    grp = n * 5 + groups * 16 + cont_groups * 24
    cls = n * 1 + ns * 4 + groups * 16 + nev * 6 + ns * 2
    emit = nev * 25 + cont_groups * 24 + ns * 33
    return {"pack": pack, "code": code, "summary": summary, "groups": grp, "class": cls, "emit": emit,
            "total": pack + code + summary + grp + cls + emit}


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--rows", type=int, default=ROWS)
    p.add_argument("--reps", type=int, default=REPS)
    a = p.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_traceloop: needs a GPU")
    igx = importlib.import_module("inspektor-gadget_amd")
    import traceloop_ref as R
    E, H = igx.engine, igx.columns
    cols, groups = build_stream(torch, a.rows)
    ns, nc = int(cols["mono_ts"].numel()), int(cols["c_mono_ts"].numel())
    n = ns + nc
    join = lambda c: E.traceloop_join(c["mono_ts"], c["sort_ts"], c["typ"], c["id"], c["pid"], valid=c["valid"],   # noqa: E731
                                      mntns=c["mntns"], c_mono_ts=c["c_mono_ts"], c_index=c["c_index"],
                                      c_mntns=c["c_mntns"], nr=NR, sync=False)
    # the yardstick's rows: the same timestamps as its key, random kinds
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    req = torch.cat([cols["mono_ts"].view(torch.int64), cols["c_mono_ts"].view(torch.int64)]).view(torch.uint64)
    kind = torch.randint(0, 3, (n,), generator=g, device="cuda").to(torch.uint8)
    yard = lambda: E.req_join(req, kind, req, sync=False)   # noqa: E731
    t_join, t_yard = [], []
    for rep in range(WARMUP + a.reps):
        tj, j = timed(torch, lambda: join(cols))
        ty, _ = timed(torch, yard)
        if rep >= WARMUP:
            t_join.append(tj)
            t_yard.append(ty)
    nev = int(H.host(j["n_events"])[0])
    cls = j["cls"][:nev]
    classes = [int((cls == k).sum()) for k in range(3)]
    with_conts = int((j["cont"][:nev] != -1).any(dim=1).sum())
    med = lambda t: sorted(t)[len(t) // 2]   # noqa: E731
    mj, my = med(t_join), med(t_yard)
    b = bytes_per_call(ns, nc, groups, nev, with_conts)
    # a sample against the row-by-row restatement
    k = min(SAMPLE, ns)
    kc = int((cols["c_mono_ts"].view(torch.int64) <= cols["mono_ts"].view(torch.int64)[:k].max()).sum())
    sub = {c: (v[:kc] if c.startswith("c_") else v[:k]) for c, v in cols.items()}
    js = E.traceloop_join(sub["mono_ts"], sub["sort_ts"], sub["typ"], sub["id"], sub["pid"], valid=sub["valid"],
                          mntns=sub["mntns"], c_mono_ts=sub["c_mono_ts"], c_index=sub["c_index"], c_mntns=sub["c_mntns"], nr=NR)
    h = {c: H.host(v) for c, v in sub.items()}
    want = R.join(h["mono_ts"], h["sort_ts"], h["typ"], h["id"].view(np.uint16), h["pid"], h["valid"], h["mntns"],
                  h["c_mono_ts"], h["c_index"], None, h["c_mntns"], NR)
    same = (js["n_events"] == len(want[0]) and
            np.array_equal(H.host(js["row"]).view(np.uint32), np.asarray(want[0], np.uint32)) and
            np.array_equal(H.host(js["exit"]).view(np.uint32), np.asarray(want[1], np.uint32)) and
            np.array_equal(H.host(js["cls"]), np.asarray(want[2], np.uint8)) and
            np.array_equal(H.host(js["cont"]).reshape(-1).view(np.uint32), np.asarray(want[3], np.uint32)))
    out = {"syscall_rows": ns, "cont_rows": nc, "containers": MNTNS, "groups": groups, "events": nev,
           "complete": classes[0], "incomplete_enter": classes[1], "incomplete_exit": classes[2],
           "events_with_conts": with_conts, "collide": COLLIDE, "lost": LOST, "reps": a.reps,
           "traceloop_join_median_ms": round(mj, 3), "traceloop_join_min_ms": round(min(t_join), 3),
           "traceloop_join_max_ms": round(max(t_join), 3),
           "req_join_rows": n, "req_join_median_ms": round(my, 3), "req_join_min_ms": round(min(t_yard), 3),
           "req_join_max_ms": round(max(t_yard), 3), "ratio_traceloop_over_req_join": round(mj / my, 3),
           "rows_per_s": round(n / (mj * 1e-3)),
           "own_pass_bytes": b, "own_pass_bytes_per_row": round(b["total"] / n, 2),
           "own_pass_ms_at_8TBps": round(b["total"] / HBM_BYTES_PER_S * 1e3, 3),
           "share_of_8TBps_own_pass_bytes_over_whole_call": round(b["total"] / (mj * 1e-3) / HBM_BYTES_PER_S, 4),
           "sample_rows": k, "sample_matches_restatement": bool(same), "device": torch.cuda.get_device_name(0),
           "note": "measured values, not targets; the two sorts' traffic is not in own_pass_bytes"}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("bench_traceloop: the device join differs from the restatement on the sample")


if __name__ == "__main__":
    main()
