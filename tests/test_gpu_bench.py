"""gpu: `bench.py` on one card, a plain run against a `--full` run of the same arguments.  The plain line carries the
headline and nothing measured outside the timed block; `--full` adds the instrumented pass (`roofline`, `kernels`), the
single-video latency and the M = 8 and OV-7B-width extras, and times the same steps: both dump the same outputs.  The
CPU baseline is left out here (`--no-cpu-baseline`); `test_bench_cpu.py` pins its code path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels", "single_video_latency_ms", "single_video_latency_graph_ms", "m8_checkpoint_shape",
             "ov7b_width_configs2", "cpu_baseline")


def _bench(args, out_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MAVLM_BENCH_M8", "MAVLM_BENCH_OV7B"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)] + args, capture_output=True, text=True, timeout=900, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench([], tmp_path / "plain")
    full = _bench(["--full", "--no-cpu-baseline"], tmp_path / "full")
    for out in (plain, full):
        assert all(k in out for k in HEADLINE), out.keys()
        assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
        assert out["fused_layernorm_exchange"]["timeouts"] == 0
    assert plain["config"]["full"] is False and full["config"]["full"] is True
    assert not [k for k in FULL_ONLY if k in plain]
    assert {k: full[k] for k in HEADLINE if k not in ("value", "ms_per_step")} == \
           {k: plain[k] for k in HEADLINE if k not in ("value", "ms_per_step")}
    assert full["roofline"]["achieved"] > 0 and full["kernels"]["attention_fwd"]["launches_per_step"] > 0
    assert full["single_video_latency_ms"] > 0 and full["single_video_latency_graph_ms"] > 0
    assert full["m8_checkpoint_shape"]["frames_per_s"] > 0
    assert "error" not in full["ov7b_width_configs2"], full["ov7b_width_configs2"]
    assert "cpu_baseline" not in full
    # the timed steps are the same in both runs: the last step's token blocks agree bit for bit but for at most a handful
    # of elements, each within 2 bf16 ulps (other inputs or another workload would differ almost everywhere)
    names = sorted(plain["dumped_outputs"]["arrays"])
    assert names == sorted(full["dumped_outputs"]["arrays"]) and len(names) == 4
    for n in names:
        a, b = np.load(tmp_path / "plain" / f"{n}.npy"), np.load(tmp_path / "full" / f"{n}.npy")
        assert a.shape == b.shape, n
        ne = a != b
        assert ne.sum() <= 16 and np.all(np.abs(a - b)[ne] <= 2.0 ** -6 * np.abs(b)[ne]), (n, int(ne.sum()))
