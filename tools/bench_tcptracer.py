"""Time igx_chain_join (trace tcp's join through two chained maps) on one GPU, against
the two igx_lw_join calls on the same two key columns that it composes, and igx_tcp_classify and the
intern step of the tuples beside it.

The stream is synthetic, built on the device as the probes' raw rows and put in timestamp order:
N_CONN connects start STEP_NS apart, connect i on thread i mod THREADS (the kprobe row at its start,
the kretprobe row RET_MIN..RET_MAX ns later, which is less than the THREADS x STEP_NS a thread
takes to come round again), on one of TUPLES sockets (IPv4, the socket's number in the source
address).  FAIL_SHARE of the connects return an error and have no later rows.  FILTERED_SHARE run
in a mount namespace outside the 64-id filter: their kprobe row is dropped at entry while their
other rows arrive.  The others see tcp_set_state(ESTABLISHED) EST_MIN..EST_MAX ns after the return
and tcp_set_state(CLOSE) LIFE_MIN..LIFE_MAX ns after that.  STRAY_SHARE x N_CONN more ESTABLISHED
rows belong to sockets nobody here connected (accepted connections).  So the rows are about
4 x N_CONN.

igx_tcp_classify turns the raw rows into kinds and tuples, a fresh engine.Interner(40) turns the
tuples of the PASS / TAKE / DROP rows into key2, and igx_chain_join joins.  The comparison runs
igx_lw_join twice: on key1 with ENTER -> SET_A, PASS / ABORT -> TAKE_A and on key2 with PASS ->
SET_A, TAKE / DROP -> TAKE_A -- the same sorts and scans without the hand-over (so its second join
admits every PASS; it is the work, not the answer).

Timing: HIP events around each call after WARMUP rounds, REPS rounds, the chain join and the two
plain joins alternating within a round, then classify and the intern step in the same round;
median and spread of each; a join's call includes its host reads (one digit plan per sort).  The
device result on the first HOST_ROWS rows is checked against tests/tcptracer_ref.py.  Prints one
JSON line (and writes it to --out).  --rounds 1 --no-check is the form a kernel trace wraps.
    python tools/bench_tcptracer.py [--out profiles/tcptracer/bench_tcptracer.json]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_CONN = 1 << 23
THREADS = 1 << 15
TUPLES = 1 << 22
STEP_NS = 100
RET_MIN, RET_MAX = 1000, 3_000_000            # below THREADS x STEP_NS = 3 276 800
EST_MIN, EST_MAX = 1000, 200_000
LIFE_MIN, LIFE_MAX = 100_000, 50_000_000
FAIL_SHARE, FILTERED_SHARE, STRAY_SHARE = 0.03, 0.02, 0.02
MNTNS_BASE, MNTNS_IDS = 4026532000, 64
WARMUP, REPS = 2, 10
HOST_ROWS = 1 << 19


def build_stream(torch, A, n_conn, threads, tuples, dev="cuda"):
    """The raw probe columns (engine.TCP_ROW_FIELDS) in timestamp order, and the filter set."""
    g = torch.Generator(device=dev)
    g.manual_seed(0x7C9)
    i = torch.arange(n_conn, dtype=torch.int64, device=dev)
    t0 = i * STEP_NS
    t_ret = t0 + torch.randint(RET_MIN, RET_MAX, (n_conn,), generator=g, device=dev)
    t_est = t_ret + torch.randint(EST_MIN, EST_MAX, (n_conn,), generator=g, device=dev)
    t_clo = t_est + torch.randint(LIFE_MIN, LIFE_MAX, (n_conn,), generator=g, device=dev)
    u = torch.rand(n_conn, generator=g, device=dev)
    fail, filtered = u < FAIL_SHARE, (u >= FAIL_SHARE) & (u < FAIL_SHARE + FILTERED_SHARE)
    ok = i[~fail]
    n_stray = int(n_conn * STRAY_SHARE)
    stray_t = torch.randint(0, n_conn * STEP_NS, (n_stray,), generator=g, device=dev)
    stray_sock = torch.randint(0, tuples, (n_stray,), generator=g, device=dev) + tuples      # nobody's socket
    sock = (i * 2654435761) % tuples
    # sections: kprobe, kretprobe, established, close, stray established
    ts = torch.cat([t0, t_ret, t_est[ok], t_clo[ok], stray_t])
    conn = torch.cat([i, i, ok, ok, torch.zeros(n_stray, dtype=torch.int64, device=dev)])
    sk = torch.cat([sock, sock, sock[ok], sock[ok], stray_sock])
    sizes = [n_conn, n_conn, ok.numel(), ok.numel(), n_stray]
    probes = [A.TCP_CONNECT_ENTER, A.TCP_CONNECT_RETURN, A.TCP_SET_STATE, A.TCP_SET_STATE, A.TCP_SET_STATE]
    states = [0, 0, 1, 7, 1]
    probe = torch.cat([torch.full((m,), p, dtype=torch.uint8, device=dev) for m, p in zip(sizes, probes)])
    state = torch.cat([torch.full((m,), s, dtype=torch.uint8, device=dev) for m, s in zip(sizes, states)])
    in_task = torch.cat([torch.ones(2 * n_conn, dtype=torch.bool, device=dev),
                         torch.zeros(2 * ok.numel() + n_stray, dtype=torch.bool, device=dev)])
    del t0, t_ret, t_est, t_clo, u, stray_t, stray_sock, sock
    ts, order = torch.sort(ts, stable=True)
    probe, state, conn, sk, in_task = probe[order], state[order], conn[order], sk[order], in_task[order]
    del order
    n = int(ts.numel())
    thread = conn % threads
    # tcp_set_state runs in some other context: tid 7 of pid 7 in the host's mount namespace
    tid = torch.where(in_task, thread + 2000, torch.full_like(thread, 7))
    pid = torch.where(in_task, thread // 4 + 1000, torch.full_like(thread, 7))
    mntns = torch.where(in_task, torch.where(filtered[conn], MNTNS_BASE + 2 * MNTNS_IDS + 1, MNTNS_BASE + 2 * (thread % MNTNS_IDS)),
                        torch.full_like(thread, 4026531840))
    ret = torch.where((probe == A.TCP_CONNECT_RETURN) & fail[conn], -111, 0).to(torch.int32)
    saddr = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    saddr[:, 0] = (0x0A000000 | sk).to(torch.int32)             # non-zero, one per socket
    daddr = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    daddr[:, 0] = 0x0A010001
    rows = {"probe": probe, "tid": tid.to(torch.int32), "pid": pid.to(torch.int32),
            "uid": (thread % 5).to(torch.int32), "mntns": mntns, "ret": ret, "state": state,
            "family": torch.full((n,), 2, dtype=torch.int16, device=dev),
            "netns": torch.full((n,), 4026531992 - (1 << 32), dtype=torch.int32, device=dev),
            "saddr": saddr.view(torch.uint8), "daddr": daddr.view(torch.uint8),
            "dport": torch.full((n,), 0x5000, dtype=torch.int16, device=dev),
            "sport": (1 + (sk & 0x3FFF)).to(torch.int16), "num": torch.zeros(n, dtype=torch.int16, device=dev)}
    ns = MNTNS_BASE + 2 * torch.arange(MNTNS_IDS, dtype=torch.int64, device=dev)
    return rows, ns, ts


def _stats(t):
    t = sorted(t)
    return round(t[len(t) // 2], 3), round(t[0], 3), round(t[-1], 3)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--connects", type=int, default=N_CONN)
    p.add_argument("--threads", type=int, default=THREADS)
    p.add_argument("--tuples", type=int, default=TUPLES)
    p.add_argument("--rounds", type=int, default=REPS)
    p.add_argument("--no-check", action="store_true")
    a = p.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tcptracer: needs a GPU")
    igx = importlib.import_module("inspektor-gadget_amd")
    import tcptracer_ref as R
    E, H, A = igx.engine, igx.columns, igx._abi
    rows, ns, _ = build_stream(torch, A, a.connects, a.threads, a.tuples)
    n = int(rows["probe"].numel())

    def classify():
        return E.tcp_classify(rows, mntns_set=ns)

    def keyed_mask(kind):
        return ((kind == A.CJ_PASS) | (kind == A.CJ_TAKE) | (kind == A.CJ_DROP)).to(torch.uint8)

    cl = classify()
    kind, key1 = cl["kind"], cl["key1"]
    keyed = keyed_mask(kind)
    it = E.Interner(A.TCP_TUPLE_BYTES, n)
    key2 = it.add(cl["tuple"], keyed).to(torch.int64)
    n_tuples = it.count()
    it.destroy()
    lut1 = torch.full((256,), 255, dtype=torch.uint8, device="cuda")
    lut2 = lut1.clone()
    lut1[A.CJ_ENTER], lut1[A.CJ_PASS], lut1[A.CJ_ABORT] = A.LW_SET_A, A.LW_TAKE_A, A.LW_TAKE_A
    lut2[A.CJ_PASS], lut2[A.CJ_TAKE], lut2[A.CJ_DROP] = A.LW_SET_A, A.LW_TAKE_A, A.LW_TAKE_A
    kind_a, kind_b = lut1[kind.to(torch.int64)], lut2[kind.to(torch.int64)]
    counts = {k: int((kind == v).sum()) for k, v in (("enter", A.CJ_ENTER), ("pass", A.CJ_PASS), ("abort", A.CJ_ABORT),
                                                     ("take", A.CJ_TAKE), ("drop", A.CJ_DROP))}
    t_cj, t_lw, t_cl, t_in = [], [], [], []
    warm = min(WARMUP, a.rounds - 1)
    for rep in range(warm + a.rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        ev[0].record()
        j = E.chain_join(key1, key2, kind, sync=False)
        ev[1].record()
        ev[2].record()
        ja = E.lw_join(key1, kind_a, sync=False)
        jb = E.lw_join(key2, kind_b, sync=False)
        ev[3].record()
        ev[4].record()
        c2 = classify()
        ev[5].record()
        it = E.Interner(A.TCP_TUPLE_BYTES, n)
        ev[6].record()
        ids = it.add(c2["tuple"], keyed)
        ev[7].record()
        torch.cuda.synchronize()
        it.destroy()
        if rep >= warm:
            t_cj.append(ev[0].elapsed_time(ev[1]))
            t_lw.append(ev[2].elapsed_time(ev[3]))
            t_cl.append(ev[4].elapsed_time(ev[5]))
            t_in.append(ev[6].elapsed_time(ev[7]))
        nt, npend = int(j["n_take"].cpu().view(torch.int64)), int(j["n_pend"].cpu().view(torch.int64))
        n_a, n_b = int(ja["n_take"].cpu().view(torch.int64)), int(jb["n_take"].cpu().view(torch.int64))
        del j, ja, jb, c2, ids
    same = None
    if not a.no_check:
        m = min(HOST_ROWS, n)
        host_rows = {k: H.host(v[:m]) for k, v in rows.items()}
        for k in ("tid", "pid", "uid", "netns"):
            host_rows[k] = host_rows[k].view(np.uint32)
        for k in ("family", "dport", "sport", "num"):
            host_rows[k] = host_rows[k].view(np.uint16)
        host_rows["mntns"] = host_rows["mntns"].view(np.uint64)
        want = R.classify(host_rows, mntns=H.host(ns).view(np.uint64))
        same = bool(np.array_equal(H.host(kind[:m]), want["kind"]) and
                    np.array_equal(H.host(cl["tuple"][:m]), want["tuple"]))
        k2 = H.host(key2[:m])
        take, pas, live = R.chain_join_arrays(want["key1"], k2, want["kind"])
        js = E.chain_join(key1[:m], key2[:m], kind[:m])
        same = same and all(np.array_equal(H.host(js[k]).view(np.uint32), w) for k, w in
                            (("take", take), ("pass", pas), ("pend", live)))
    (cj, cj_lo, cj_hi), (lw, lw_lo, lw_hi) = _stats(t_cj), _stats(t_lw)
    (tc, tc_lo, tc_hi), (ti, ti_lo, ti_hi) = _stats(t_cl), _stats(t_in)
    out = {"rows": n, "connects": a.connects, "threads": a.threads, "sockets": a.tuples, "distinct_tuples": n_tuples,
           "fail_share": FAIL_SHARE, "filtered_share": FILTERED_SHARE, "stray_share": STRAY_SHARE, "kinds": counts,
           "n_take": nt, "n_pend": npend, "lw_join_key1_n_take": n_a, "lw_join_key2_n_take": n_b, "rounds": a.rounds,
           "chain_join_median_ms": cj, "chain_join_min_ms": cj_lo, "chain_join_max_ms": cj_hi,
           "two_lw_joins_median_ms": lw, "two_lw_joins_min_ms": lw_lo, "two_lw_joins_max_ms": lw_hi,
           "chain_over_two_lw": round(cj / lw, 4), "chain_join_rows_per_s": round(n / (cj * 1e-3)),
           "tcp_classify_median_ms": tc, "tcp_classify_min_ms": tc_lo, "tcp_classify_max_ms": tc_hi,
           "intern_add_median_ms": ti, "intern_add_min_ms": ti_lo, "intern_add_max_ms": ti_hi,
           "intern_over_chain": round(ti / cj, 4), "sample_matches_restatement": same,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if same is False:
        raise SystemExit("bench_tcptracer: the device result differs from the restatement on the sample")


if __name__ == "__main__":
    main()
