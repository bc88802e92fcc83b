"""bench.py driver contract at world size 2 (gloo on the CPU): the launch the
driver uses for N>1 (torch.distributed.run, one rank per device) prints ONE
JSON line from rank 0 with the whole-job value and the dp degree."""
import json
import os
import sys

import pytest

from _mp import ROOT, torchrun


@pytest.mark.parametrize("world,baseline", [(2, 85.9), (8, 213.3)])
def test_bench_multi_rank_json_contract(tmp_path, world, baseline):
    """world 8: the driver's N=8 scaling launch, rehearsed on gloo."""
    out = torchrun([os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "5", "--warmup", "1", "--full"],
                   world, str(tmp_path), timeout=600)
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["steps"] == 5 and d["warmup"] == 1
    assert d["config"]["parallelism"] == f"dp{world}" and d["config"]["global_batch"] == 1440
    assert d["config"]["per_gpu_batch"] == 1440 // world and d["scaling"] == "strong"
    # the headline is the reference's metric: whole epochs (the short last
    # batch included) of epoch_sequences each, over the timed wall time
    assert d["steps_per_epoch"] == 5 and d["epochs"] == 1.0 and d["epoch_sequences"] == 6912
    assert d["timed_sequences"] == 6912 * d["epochs"]
    assert d["value"] > 0 and abs(d["value"] - d["epoch_sequences"] * d["epochs"] /
                                  (d["epoch_time_s"] * d["epochs"])) / d["value"] < 1e-3
    assert abs(d["value"] - d["timed_sequences"] / (d["ms_per_step"] * 5e-3)) / d["value"] < 1e-2
    assert d["step_seq_per_s"] > 0
    assert d["vs_baseline"] == round(d["value"] / baseline, 2)
    assert d["final_loss"] == d["final_loss"]


def test_bench_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """A plain run times --steps steps and nothing else (the full-batch-only
    figure is --full's); --dump-outputs writes the last timed step's
    statistics and the parameters it left as float32 .npy, identical from run
    to run with the same arguments."""
    import numpy as np
    from _mp import cpu_env, run

    def bench(name):
        out = run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                   "--global-batch", "96", "--epoch-sequences", "240", "--seq-len", "16", "--hidden", "8",
                   "--dump-outputs", str(tmp_path / name)], str(tmp_path), env=cpu_env())
        lines = [ln for ln in out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out[-3000:]
        return json.loads(lines[0]), {p.name: np.load(p) for p in sorted((tmp_path / name).iterdir())}

    d, a = bench("a")
    assert d["steps"] == 4 and d["steps_per_epoch"] == 3 and d["timed_sequences"] == 240 + 96
    assert d["ms_per_step"] > 0 and d["unit"] == "sequences/s" and d["higher_is_better"] is True
    assert abs(d["value"] - d["timed_sequences"] / (d["ms_per_step"] * 4e-3)) / d["value"] < 1e-2
    assert "step_seq_per_s" not in d and "step_ms_full_batch" not in d
    assert set(a) == {"stats.npy"} | {f"param.{n}.npy" for n in (
        "fc.weight", "fc.bias", *(f"lstm.{w}_{g}_l{k}" for w in ("weight", "bias") for g in ("ih", "hh") for k in (0, 1)))}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["param.lstm.weight_hh_l1.npy"].shape == (32, 8)
    # the last timed step is the first batch of the second epoch: 96 sequences
    assert a["stats.npy"].shape == (3,) and a["stats.npy"][1] == 96
    assert abs(float(a["stats.npy"][0]) - d["final_loss"]) < 1e-5
    _, b = bench("b")
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
