"""bench.py on one GPU with a small workload: a plain run times exactly --steps steps and leaves the checking
legs out, --full brings them back, and --dump-outputs writes the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--docs-per-gpu", "96", "--ops", "400"]
NAMES = ("replay_stats", "doc_digests", "sample_docs", "sample_dump_fnv", "sample_text_offsets", "sample_text")


def _bench(args):
    env = dict(os.environ)
    for k in ("MTB_NO_TORCH", "MTB_LOG_CACHE", "WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump_a")
    return _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(d)]), d


def test_plain_run_times_the_steps_it_was_given(plain):
    out, _ = plain
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["unit"] == "ops/s" and out["higher_is_better"] is True and out["dtype"] == "int32"
    assert out["ms_per_step"] > 0
    # value = ops of the timed steps / their wall time, ms_per_step = that wall time / steps
    ops = out["config"]["ops_per_step"]
    assert ops > 96 * 400 * 0.9
    assert out["value"] == pytest.approx(ops / (out["ms_per_step"] * 1e-3), rel=1e-3)
    # the legs with runs or passes of their own stay out of a plain run
    for k in ("parity", "snapshot_v1", "cpu_baseline", "traffic_pmc"):
        assert out[k] is None, k
    assert out["roofline"]["traffic"] is None and out["roofline"]["kernel"]


def test_dump_outputs_are_float_arrays_of_the_last_step(plain):
    out, d = plain
    assert sorted(os.listdir(d)) == sorted(f"{n}.npy" for n in NAMES)
    a = {n: np.load(os.path.join(d, f"{n}.npy")) for n in NAMES}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    st = a["replay_stats"]
    assert st[0] == out["config"]["ops_per_step"] and st[1] == 96 and st[2] == 0 and st[4] > 0 and st[5] > 0
    assert a["doc_digests"].shape == (96, 4) and a["doc_digests"].max() <= 0xFFFF
    assert len(np.unique(a["doc_digests"], axis=0)) == 96  # every document has a log of its own
    k = len(a["sample_docs"])
    assert k == 64 and a["sample_dump_fnv"].shape == (k, 4)
    off = a["sample_text_offsets"]
    assert len(off) == k + 1 and off[0] == 0 and off[-1] == a["sample_text"].size and np.all(np.diff(off) >= 0)


def test_dump_outputs_repeat_and_full_checks_them(plain, tmp_path):
    """A second run with the same workload options (other step counts, --full) writes the same arrays, and its
    parity legs find every document equal to the oracle's."""
    _, d = plain
    out = _bench(["--steps", "1", "--warmup", "0", "--full", "--no-cpu", "--traffic", "off", "--dump-outputs",
                  str(tmp_path)])
    assert out["steps"] == 1
    assert out["parity"]["sampled_docs"] == 96 and out["parity"]["mismatches"] == 0 and out["parity"]["errors"] == 0
    assert out["parity"]["dump_checksum_mismatches"] == 0
    assert out["snapshot_v1"]["documents"] == 96 and out["snapshot_v1"]["mismatches"] == 0
    for n in NAMES:
        assert np.array_equal(np.load(os.path.join(d, f"{n}.npy")), np.load(tmp_path / f"{n}.npy")), n
