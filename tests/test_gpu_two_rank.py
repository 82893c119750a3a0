"""The N > 1 TS-VAD path with the real HIP forward (round-4 verdict item 7): `bench.py`'s strong-scaling
`main()` as two ranks on the one leased GPU (gloo process group, every rank on cuda:0:
tests/bench_main_gpu_ranks.py) against one rank, on a 13-min C4 meeting (CAM++ + transformer, rs_len 4):
~390 windows per rank, so each rank's device call runs the two-stream window slices.  The 2-rank posteriors
must equal the 1-rank posteriors bit for bit (every rank holds the gathered meeting).  SDIAR_NO_LSTM_SEQ is
not needed (C4 has no BiLSTM); it is set anyway so a v1 run would not depend on co-residency."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--workload", "c4", "--minutes", "13", "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
        "--no-kernel-timing", "--full"]


def _port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, out):
    port = str(_port())
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port, SDIAR_NO_LSTM_SEQ="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "bench_main_gpu_ranks.py"), out,
                                       *ARGS], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                      cwd=REPO))
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, o, e))
    for rc, o, e in outs:
        assert rc == 0, e[-3000:]
    lines = [ln for ln in outs[0][1].splitlines() if ln.startswith("{")]
    assert len(lines) == 1, outs[0][1][-2000:]
    assert not any(ln.startswith("{") for _, o, _ in outs[1:] for ln in o.splitlines()), "only rank 0 prints"
    return json.loads(lines[0])


def test_two_ranks_on_one_gpu_match_one_rank(gpu, tmp_path):
    d1, d2 = tmp_path / "w1", tmp_path / "w2"
    d1.mkdir()
    d2.mkdir()
    one = _run(1, str(d1))
    two = _run(2, str(d2))
    print("1 rank:", one["ms_per_step"], "ms; 2 ranks on one GPU:", two["ms_per_step"], "ms")
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2 and two["rccl_ranks"] == [0, 1]
    assert two["config"]["windows"] == one["config"]["windows"] >= 768
    assert "window-shard x2" in two["config"]["parallelism"]
    p1 = np.load(d1 / "post_rank0.npy")
    assert np.isfinite(p1[:, : p1.shape[1] - 200]).all()
    for r in range(2):
        np.testing.assert_array_equal(np.load(d2 / f"post_rank{r}.npy"), p1)
