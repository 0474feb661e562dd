"""bench.py's CPU-side helpers (no GPU): the `cpu_baseline` legs of the three reference calls a --full run times at the configs' shapes —
eval_tree_array (C2), eval_grad_tree_array(variable=true) (C3), the ParametricExpression eval + constant-mode gradient (C5) — on tiny inputs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import dynamicexpressions_jl_amd as de  # noqa: E402


def test_cpu_baseline_kinds_time_the_reference_calls_of_the_configs():
    ops = de.synth.BENCH_OPERATORS
    X = de.synth.random_X(5, 4000, seed=1)
    trees = de.synth.random_population(24, seed=0xDE02)
    for kind in ("eval", "grad"):
        r = bench.cpu_baseline(trees, ops, X, 0.5, 0.25, kind=kind)
        assert r["kind"] == "port" and r["value"] > 0 and r["cores"] >= 1 and r["single_thread"]["cores"] == 1
        assert ("eval_grad_tree_array" in r["sample"]) == (kind == "grad")
    pt = de.synth.random_population(24, seed=0xDE05, node_type=de.ParametricNode, nparams=8)
    g = np.random.default_rng(0)
    params = np.asfortranarray(g.standard_normal((8, 16)).astype(np.float32))
    classes = g.integers(1, 17, 4000).astype(np.int32)
    r = bench.cpu_baseline(pt, ops, X, 0.5, 0.0, kind="param", params=params, classes=classes)
    assert r["value"] > 0 and "single_thread" not in r and "ParametricExpression" in r["sample"]


def test_default_run_lists_every_baseline_config():
    """the `configs` legs of a --full run = BASELINE.json's configs 2-5 (config 4 as rank 0's shard, config 5 in its three readings)"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'for k in ("C2", "C3", "C4", "C5", "C5N", "C5Ng", "C5pb")' in src
    for k in ("C2", "C3", "C4", "C5", "C5N", "C5Ng", "C5pb"):
        assert k in bench.WORKLOADS
    assert bench.WORKLOADS["C4"]["shards"] == 8 and bench.WORKLOADS["C4"]["n_trees"] * 8 == 10000
    assert bench.WORKLOADS["C5pb"].get("reverse_grad") is True  # (reverse accumulation is an opt-in since ABI 3: the workload that measures it says so)


def test_dump_writer_keeps_to_float_arrays_within_the_bound(tmp_path):
    """--dump-outputs: one DIR/<name>.npy per array, finite float32 / float64 only, DUMP_BYTES in all (files, headers included)"""
    arrs = {"ok": np.array([1, 0, 1], dtype=np.float32), "out": np.arange(12, dtype=np.float32).reshape(3, 4),
            "samples": np.array([0, 5, 9, 11], dtype=np.float64)}
    assert bench.write_outputs(str(tmp_path / "d"), arrs) == {"ok": [3], "out": [3, 4], "samples": [4]}
    for name, a in arrs.items():
        b = np.load(tmp_path / "d" / f"{name}.npy")
        assert b.dtype == a.dtype and np.array_equal(a, b)
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "e"), {"ok": np.array([1, 0], dtype=np.uint8)})
    for bad in (np.nan, np.inf):
        with pytest.raises(AssertionError):
            bench.write_outputs(str(tmp_path / "g"), {"out": np.array([1.0, bad], dtype=np.float32)})
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "f"), {"out": np.zeros(bench.DUMP_BYTES // 4, dtype=np.float32)})


@pytest.mark.gpu
def test_dump_outputs_are_the_same_for_any_number_of_steps(tmp_path):
    """`bench.py --dump-outputs DIR` on the GPU: the last timed step's outputs, identical whatever --steps (the inputs are seeded), float
    only, finite and within the bound; the rows of incomplete trees (unspecified) are 0, those of complete trees are what the kernel
    wrote, finite without any replacement (their sum is: the reference's flag)."""
    import json
    import subprocess
    dumps = []
    for steps in (1, 3):
        d = tmp_path / f"s{steps}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                            "--no-cpu-baseline", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert line["outputs_dumped"]["shapes"] == {"ok": [64], "samples": [10**5], "out": [64, 10**5]}
        assert line["outputs_dumped"]["nonfinite_written_as_zero"] == {}
        files = sorted(os.listdir(d))
        assert files == ["ok.npy", "out.npy", "samples.npy"] and sum(os.path.getsize(d / f) for f in files) <= bench.DUMP_BYTES
        dumps.append({f: np.load(d / f) for f in files})
    for f, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and np.array_equal(a, dumps[1][f]), f
    ok, out = dumps[0]["ok.npy"].astype(bool), dumps[0]["out.npy"]
    assert 0 < ok.sum() < len(ok) and (out[~ok] == 0).all()


@pytest.mark.gpu
def test_plain_run_does_the_timed_steps_only_and_full_adds_the_legs():
    """A plain `bench.py` run warms up, times the steps and prints the line; `--full` adds the secondary legs on top of the same line."""
    import json
    import subprocess
    lines = []
    for extra in ([], ["--full", "--no-cpu-baseline"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--gpus", "1", "--steps", "2", "--warmup", "1"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    plain, full = lines
    for d in (plain, full):
        assert d["metric"] == "node-evals/sec" and d["unit"] == "node-evals/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["roofline"]["frac"] > 0
    legs = ("turbo", "full_evaluation", "complete_only", "dataset_declared", "rounds_1_4_x", "forward_default", "search_generation",
            "cpu_baseline", "configs", "wide_x")
    assert not [k for k in legs if k in plain]
    assert all(k in full for k in ("turbo", "full_evaluation", "dataset_declared"))
    assert plain["config"]["complete_fraction"] == full["config"]["complete_fraction"]
