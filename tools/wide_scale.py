"""Measurement: one wide table at scale.  An interval of top tcp's key (ip_key_t) over --keys
distinct keys (default 12M: past the 8.39M groups a narrow table holds) runs in AUTO on a table of
capacity 2^24 (2^25 slots x 128 B = 4 GiB of key records, a wide table; --capacity 16777217: 8 GiB)
and is compared with the all-cores oracle (or_top_tcp_mt) on the same stream: group count,
whole-table checksum and the top-20 by -sent, -recv.  AUTO runs it partitioned.  The interval is
fed twice: the first time also allocates the partitioned form's scratch (wall time reported), the
second is timed once with HIP events and checked.  Not part of the product path or the tests.

    python tools/wide_scale.py [--keys 12000000] [--events 48000000] [--zipf 0.2] [--capacity N]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("saddr", "daddr", "mntns", "pid", "comm", "lport", "dport", "family", "size", "dir")


def u64_col(rows, off):
    return rows[:, off:off + 8].copy().view(np.uint64).ravel()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--keys", type=int, default=12_000_000)
    p.add_argument("--events", type=int, default=48_000_000)
    p.add_argument("--zipf", type=float, default=0.2)
    p.add_argument("--capacity", type=int, default=1 << 24)
    a = p.parse_args()
    import torch
    from oracle import oracle as O
    igx = importlib.import_module("inspektor-gadget_amd")
    E, H, A = igx.engine, igx.columns, igx._abi
    n, G = a.events, a.keys
    cdf_h = O.zipf_cdf(G, a.zipf)
    ev = E.gen_tcp(0xC2, 0, G, H.to_device(cdf_h), 0, n)
    cols = [ev[k] for k in NAMES]
    t0 = time.perf_counter()
    tab = E.Table([16, 16, 8, 4, 16, 2, 2, 2], [A.Agg(A.AGG_SUM, 8, 9, 8, 0), A.Agg(A.AGG_SUM, 8, 9, 8, 1)], a.capacity)
    torch.cuda.synchronize()
    create_s = time.perf_counter() - t0
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    # the first interval also allocates the partitioned form's scratch (host time between the two
    # events); the second is the steady state, and the one compared with the oracle
    t0 = time.perf_counter()
    tab.update(cols, list(range(8)), n, 0)
    torch.cuda.synchronize()
    first_s = time.perf_counter() - t0
    tab.reset()
    e0.record()
    tab.update(cols, list(range(8)), n, 0)
    e1.record()
    fin = tab.finalize()
    top = tab.gather(tab.sort([(A.TSRC_AGG, 0, True), (A.TSRC_AGG, 1, True)], 20))
    e2.record()
    torch.cuda.synchronize()
    out = {"keys": G, "events": n, "zipf": a.zipf, "capacity": a.capacity,
           "key_record_bytes": fin["n_slots"] * fin["key_stride"], "form": tab.info()["form"],
           "region": tab.info()["region"], "create_s": round(create_s, 3),
           "first_interval_wall_s": round(first_s, 3),
           "update_ms": round(e0.elapsed_time(e1), 3), "finalize_topk_ms": round(e1.elapsed_time(e2), 3),
           "groups": fin["n_groups"]}
    slots = torch.empty(fin["n_groups"], dtype=torch.int32, device="cuda")
    tab.ctx.check(tab.ctx.L.igx_memcpy_d2d(tab.ctx.h, slots.data_ptr(), fin["groups_ptr"], fin["n_groups"] * 4))
    out["max_slot_byte_offset"] = int(slots.to(torch.int64).max().item()) * fin["key_stride"]
    rows = H.host(tab.gather(slots))
    f66 = np.concatenate([rows[:, 0:62], rows[:, 64:66], rows[:, 68:70]], axis=1)
    dev_cs = O.tcp_group_checksum(f66, u64_col(rows, 72), u64_col(rows, 80), u64_col(rows, 88))
    del rows, f66
    top = H.host(top)
    tab.destroy()
    h = O.gen_tcp(0xC2, 0, G, cdf_h, 0, n)
    t0 = time.perf_counter()
    Gref, sent, recv, first, cs = O.top_tcp_mt(h, 20, checksum=True)
    out["oracle_s"] = round(time.perf_counter() - t0, 2)
    out["oracle_threads"] = O.cpu_threads()
    out["oracle_groups"] = int(Gref)
    out["groups_equal"] = int(Gref) == fin["n_groups"]
    out["table_checksum_equal"] = dev_cs == cs
    out["topk_equal"] = bool(np.array_equal(u64_col(top, 72), sent) and np.array_equal(u64_col(top, 80), recv) and
                             np.array_equal(u64_col(top, 88), first))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
