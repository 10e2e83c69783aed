"""bench.py's launch contract on the CPU (no GPU work): ``--gpus N`` without a torch.distributed
launcher starts N ranks itself (torch.distributed.run, rendezvous on 127.0.0.1), and a rank whose
WORLD_SIZE disagrees with --gpus refuses to run (VERDICT r02 "what's missing" 3)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=300)


def test_gpus_flag_spawns_one_rank_per_gpu():
    r = _run(["--gpus", "2", "--full"], {"M3S_BENCH_SPAWN_CHECK": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1]
    assert all(d["world"] == 2 for d in lines)
    assert sorted(d["local_rank"] for d in lines) == [0, 1]
    # with --full every rank also times BASELINE configs[3] (the 1024-edge cfg4 graph: 2048 directed edges),
    # edge-sharded like the headline config: the ranks' ranges tile [0, 2048)
    for cfg, n in (("cfg3", 512), ("cfg4", 2048)):
        ranges = sorted(tuple(d["edge_ranges"][cfg]) for d in lines)
        assert ranges[0][0] == 0 and ranges[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))


def test_cfg4_block_can_be_skipped():
    r = _run(["--gpus", "1", "--full", "--no-cfg4"], {"M3S_BENCH_SPAWN_CHECK": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    (d,) = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert list(d["edge_ranges"]) == ["cfg3"]


def test_plain_run_times_the_headline_config_only():
    r = _run(["--gpus", "1"], {"M3S_BENCH_SPAWN_CHECK": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    (d,) = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert list(d["edge_ranges"]) == ["cfg3"]


def test_dump_outputs_writes_one_float32_npy_per_output(tmp_path):
    import numpy as np
    import torch

    import bench

    outs = {"Twc": torch.arange(16, dtype=torch.float32).reshape(2, 8), "dx": torch.ones(1, 7)}
    d = tmp_path / "new" / "dir"
    bench.dump_outputs(str(d), outs)
    assert sorted(os.listdir(d)) == ["Twc.npy", "dx.npy"]
    for name, t in outs.items():
        a = np.load(d / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.numpy())


def test_world_size_must_match_gpus_flag():
    r = _run(["--gpus", "1"], {"M3S_BENCH_SPAWN_CHECK": "1", "WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr
