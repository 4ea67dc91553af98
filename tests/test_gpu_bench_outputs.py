"""GPU: bench.py's plain run (headline line only, --dump-outputs) and --full
(everything else the line carries) at N = 1 without a launcher."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import quant_ref as Q

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
DOCS, SEED, TOP_K, MIN_SIM = 100, 1234, 10, 0.5
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config"}
FULL_ONLY = {"roofline", "keyswitch_ms_total", "parity", "leveled_score", "pcie_inclusive", "topk_check",
             "cpu_baseline"}


def _bench(*extra):
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--docs", str(DOCS)] + list(extra)
    r = subprocess.run(cmd, cwd=str(REPO), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_step(need_gpu, tmp_path):
    """A plain run carries the headline fields and nothing that needs a run of
    its own; --dump-outputs writes the last step's accumulators, threshold
    bits and top-k as float64, equal to the clear restatement of the path on
    the inputs the arguments fix."""
    import bench
    from fheicp.datagen import training_pairs
    out = _bench("--dump-outputs", str(tmp_path / "o"))
    assert HEADLINE <= set(out) and not (FULL_ONLY & set(out)), sorted(out)
    assert out["steps"] == 2 and out["warmup"] == 1 and out["unit"] == "compares/s" and out["dtype"] == "u64"
    assert out["metric"] == bench.METRIC and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - DOCS / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    got = {n: np.load(tmp_path / "o" / f"{n}.npy") for n in ("acc", "below", "topk_acc", "topk_index")}
    assert all(a.dtype == np.float64 for a in got.values())

    class A:
        workload, dim, docs, seed = "c2", 16, DOCS, SEED
    q, docs, _ = bench.shard(A, 0)
    X, y = training_pairs(16, 1000, seed=SEED + 1)
    oq = Q.fit_quantized_linear(X, y, 6)
    acc = Q.accumulate(oq, Q.quantize_input(oq, Q.pair_features(q, docs)))
    scores = Q.dequantize(oq, acc)
    assert np.array_equal(got["acc"], acc.astype(np.float64))
    assert np.array_equal(got["below"], (scores < MIN_SIM).astype(np.float64))
    keep = [i for i in np.argsort(-scores, kind="stable") if scores[i] >= MIN_SIM][:TOP_K]
    idx = got["topk_index"]
    assert [int(i) for i in idx if i >= 0] == keep
    assert np.array_equal(got["topk_acc"][idx >= 0], acc[keep].astype(np.float64))


def test_full_run_adds_the_checks_and_side_measurements(need_gpu):
    """--full: the same headline plus the roofline, parity, the leveled and
    host-buffer timings and the top-k check (the CPU oracle baseline is
    switched off here for time)."""
    out = _bench("--full", "--no-cpu-baseline")
    assert HEADLINE <= set(out) and (FULL_ONLY - {"cpu_baseline"}) <= set(out), sorted(out)
    par = out["parity"]
    assert par["compares_checked"] == DOCS
    assert par["acc_bit_exact"] and par["threshold_bit_exact"] and par["quant_params_equal"]
    assert out["topk_check"]["indices_equal"] and out["topk_check"]["scores_equal"]
    assert out["leveled_score"]["acc_equal_to_compare"]
    assert out["roofline"]["launches"] > 0
