"""Multi-rank paths on CPU: tests/dist_worker.py under torch.distributed.run with gloo,
world_size 2 (C3 all-reduce, C4 all-to-all + owner merge, top-K
all-gather merge), checked against the oracle over the union of both ranks' events."""
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world2_gloo_merges():
    env = dict(os.environ, OMP_NUM_THREADS="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dist_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DIST_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_exchange_partitioned_rejects_the_overflow_sentinel():
    """igx_partition_groups writes UINT64_MAX into every count when the table lists more groups
    than the output holds; through the binding's int64 tensor that is -1.  exchange_partitioned
    must refuse such counts with IGX_ENOSPC before it slices or sends anything (rows[:sum(counts)]
    of negative counts would silently drop rows from the end), and pass sane counts through."""
    import importlib

    import pytest
    import torch
    D = importlib.import_module("inspektor-gadget_amd.dist")
    A = importlib.import_module("inspektor-gadget_amd._abi")
    rows = torch.arange(40, dtype=torch.uint8).reshape(10, 4)
    sentinel = torch.full((4,), -1, dtype=torch.int64)
    assert sentinel.view(torch.uint64)[0].item() == 2 ** 64 - 1
    for counts in (sentinel.tolist(), [3, -1, 2, 1], [-1]):
        with pytest.raises(A.IgxError) as ei:
            D.exchange_partitioned(rows, counts)
        assert ei.value.code == A.IGX_ENOSPC
    assert torch.equal(D.exchange_partitioned(rows, [4, 3, 0, 2]), rows[:9])   # one rank: its own rows
    assert D.exchange_partitioned(rows, [0, 0]).shape[0] == 0
