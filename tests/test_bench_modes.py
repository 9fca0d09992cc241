"""bench.py's two modes.  A plain run does only the headline's setup, warmup and timed steps
(no other config, CPU baseline, roofline clock or oracle check); `--full` keeps them all.
`--dump-outputs DIR` writes the last timed step's top-K rows and table as float .npy files:
two runs with the same arguments must write the same arrays, and they must be what the oracle
computes on the last step's own slice of the stream."""
import importlib
import json
import os
import sys

import numpy as np
import pytest


def test_plain_run_drops_everything_but_the_headline():
    bench = importlib.import_module("bench")
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.check is False and a.cpu_sample == 0 and a.configs == ""
    a = bench.parse(["--configs", "c3,c5", "--cpu-sample", "1000"])          # nothing to act on
    assert a.check is False and a.cpu_sample == 0 and a.configs == ""


def test_full_run_keeps_the_other_measurements():
    bench = importlib.import_module("bench")
    a = bench.parse(["--full"])
    assert a.full and a.check is True and a.cpu_sample == 48_000_000 and a.configs == "c1,c3,c4,c5"
    a = bench.parse(["--full", "--no-check", "--cpu-sample", "0", "--configs", "c5", "--dump-outputs", "d"])
    assert a.check is False and a.cpu_sample == 0 and a.configs == "c5" and a.dump_outputs == "d"


N, G, K, STEPS, WARMUP = 1_000_003, 50_000, 20, 3, 1


def _main(bench, monkeypatch, capsys, extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                                      "--events", str(N), "--keys", str(G)] + extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(igx, oracle, tmp_path, monkeypatch, capsys):
    bench = importlib.import_module("bench")
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _main(bench, monkeypatch, capsys, ["--dump-outputs", d1])
    _main(bench, monkeypatch, capsys, ["--dump-outputs", d2])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "events/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    assert line["metric"] == bench.METRIC
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["config"]["batches"] == STEPS + WARMUP          # one slice of the stream per interval
    assert line["configs"] == {} and "check" not in line
    assert line["cpu_baseline"] is None and line["roofline"] is None

    names = sorted(os.listdir(d1))
    assert names == sorted(n + ".npy" for n in ("n_groups", "table", "topk_first", "topk_recv", "topk_rows",
                                                "topk_sent"))
    got = {n[:-4]: np.load(os.path.join(d1, n)) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= bench.DUMP_BUDGET
    for n in names:                                             # same arguments, same inputs, same outputs
        assert np.array_equal(got[n[:-4]], np.load(os.path.join(d2, n))), n

    # the last timed interval's slice is the (STEPS + WARMUP - 1)-th of the stream
    base = (STEPS + WARMUP - 1) * N
    cdf = oracle.zipf_cdf(G, 1.1)
    h = oracle.gen_tcp(0xC2, 0, G, cdf, base, N)
    Gref, sent, recv, first, _ = oracle.top_tcp_mt(h, K, base_idx=base, threads=4, checksum=True)
    assert got["n_groups"].tolist() == [Gref]
    assert np.array_equal(got["topk_sent"], np.asarray(sent, np.uint64).astype(np.float64))
    assert np.array_equal(got["topk_recv"], np.asarray(recv, np.uint64).astype(np.float64))
    assert np.array_equal(got["topk_first"], np.asarray(first, np.uint64).astype(np.float64))
    rows = got["topk_rows"].astype(np.uint8)
    assert rows.shape == (K, 96) and np.array_equal(bench.u64_col(rows, 72).astype(np.float64), got["topk_sent"])
    t = got["table"]
    assert t.shape == (Gref, 3) and np.all(np.diff(t[:, 0]) > 0) and t[0, 0] >= base and t[-1, 0] < base + N
    # every event the probes keep is summed once: family in {2, 10}; receives (dir 1) with copied > 0
    fam, size, rx = h["family"].view(np.int16), h["size"].view(np.int32).astype(np.int64), h["dir"] == 1
    keep = ((fam == 2) | (fam == 10)) & (~rx | (size > 0))
    assert t[:, 1].sum() == float(h["size"].astype(np.uint64)[keep & ~rx].sum())
    assert t[:, 2].sum() == float(h["size"].astype(np.uint64)[keep & rx].sum())
