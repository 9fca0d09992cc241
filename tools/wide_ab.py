"""Measurement: what 64-bit record addressing costs on its own.  The bench's C4 stream (the
network-policy tuples; its table is narrow: 2^25 slots of 32 B) runs in the direct and in the
partitioned form on two tables of the same size, one created with IGX_GB_WIDE=0 and one with
IGX_GB_WIDE=1 (the wide kernel instances on a narrow-sized table), the reps interleaved; update
times are HIP events.  Group counts and first-index sums are printed so the runs can be compared.
Not part of the product path or the tests.

    python tools/wide_ab.py [--events 125000000] [--reps 5] [--forms direct,part]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--events", type=int, default=125_000_000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--forms", default="direct,part")
    a = p.parse_args()
    import torch
    igx = importlib.import_module("inspektor-gadget_amd")
    E, H, A = igx.engine, igx.columns, igx._abi
    modes = {"direct": A.GB_DIRECT, "part": A.GB_PART}
    n = a.events
    ev = E.gen_np(0xC4, 10_000, 100_000, 0, n)
    keep = E.np_mark(ev["type"], ev["pkt"], ev["hostip"], ev["raddr"])
    cols = [ev[k] for k in ("src", "pkt", "peer", "port")]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in a.forms.split(","):
        tabs = {}
        for wide in (0, 1):
            os.environ["IGX_GB_WIDE"] = str(wide)     # read by igx_groupby_create
            tabs[wide] = E.Table([4, 1, 4, 2], [], 11_000_000)
            tabs[wide].set_mode(modes[f])
        os.environ.pop("IGX_GB_WIDE")
        ts = {0: [], 1: []}
        for r in range(a.reps + 1):
            for wide in (0, 1):
                tab = tabs[wide]
                tab.reset()
                e0.record()
                tab.update(cols, [0, 1, 2, 3], n, 0, valid=keep)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    ts[wide].append(e0.elapsed_time(e1))
        out = {"form": f, "events": n}
        for wide in (0, 1):
            fin = tabs[wide].finalize()
            _, _, first = E.table_tensors(tabs[wide], fin)
            key = "wide" if wide else "narrow"
            out[key + "_ms"] = [round(t, 3) for t in ts[wide]]
            out[key + "_median_ms"] = float(np.median(ts[wide]))
            out[key + "_groups"] = fin["n_groups"]
            out[key + "_first_sum"] = int(H.host(first).astype(np.uint64).sum())
            tabs[wide].destroy()
        out["wide_over_narrow"] = round(out["wide_median_ms"] / out["narrow_median_ms"], 4)
        torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
