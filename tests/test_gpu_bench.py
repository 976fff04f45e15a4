"""bench.py as a command: a plain run times its steps and prints the headline
line only; --dump-outputs writes what the last timed step computed (checked
against the oracle); --full adds the per-round profile, the roofline and the
CPU baseline."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gossip_hip._abi import STAT_FIELDS
from gossip_hip.workloads import config

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config")
FULL_ONLY = ("rounds", "roofline", "cpu_baseline")


def _bench(*args):
    p = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(oracle, tmp_path):
    """Config 1 (8 peers, 80 messages in two words, a death, ping rounds): the plain line, and the dump of its
    last step against the oracle's run of the same workload."""
    line = _bench("--config", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "GTEPS" and line["dtype"] == "u64"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    w = config(1, pick=oracle.pick_origins)
    rp, col = oracle.gen_workload(w)
    ref = oracle.simulate_workload(w, rp, col)
    got = {p.stem: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert set(got) == {"round_stats", "coverage", "seen_peers", "seen_sample"}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert np.array_equal(got["seen_peers"], np.arange(w.n))
    bits = (ref["seen"][:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    assert np.array_equal(got["seen_sample"], bits.reshape(w.n, -1)[:, :w.n_msgs].astype(np.float32))
    assert np.array_equal(got["coverage"], ref["coverage"].astype(np.float64))
    want = [[s["round"], s["flags"]] + [v for f in STAT_FIELDS for v in
                                        ((s[f] >> 32, s[f] & 0xFFFFFFFF) if f == "digest" else (s[f],))]
            for s in ref["stats"]]
    assert np.array_equal(got["round_stats"], np.array(want, dtype=np.float64))
    assert line["config"]["rounds"] == len(ref["stats"])


def test_full_run_adds_profile_roofline_and_cpu_baseline():
    line = _bench("--full", "--config", "3", "--n", "16384", "--steps", "2", "--warmup", "1", "--cpu-sample-n", "16384",
                  "--cpu-sample-n1", "16384", "--cpu-repeats", "1")
    assert all(k in line for k in HEADLINE + FULL_ONLY)
    assert len(line["rounds"]) == line["config"]["rounds"] and line["roofline"]["timed_steps"] == 2
    assert line["cpu_baseline"]["value"] > 0
