"""The final stdout line of bench.py is what the driver parses: it must stay small (round 3's 32 KB line was not
parsed) and carry the contract's fields whatever the size of the full record."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _full_record(n_layers=17):
    rl = {"kernel": "spatial_conv_bwd", "bound": "mfma", "achieved": 90.575, "peak": 157.3, "unit": "TFLOP/s",
          "frac": 0.5758, "traffic": 1224237649, "ms": 0.366, "edges": 4543198, "mlp_blocks": 8,
          "conv_kernels": "x" * 200, "executed_frac": 0.3576,
          "fwd_bwd": {"fwd": {"ms": 0.1689, "algorithmic_frac": 0.4378, "executed_frac": 0.31},
                      "bwd": {"ms": 0.366, "algorithmic_frac": 0.5758, "executed_frac": 0.36}},
          "mfma_pipe_busy_from_committed_profile": {"bwd": {"kernel": "f1_bwd_edges", "busy": 0.24}, "fwd": {"kernel": "f", "busy": 0.31},
                                                    "source": "profiles/x.json", "kernel_sources_match": True,
                                                    "measured_in_this_run": False},
          "traffic_from_committed_profile": {"bytes": 1224237649, "source": "profiles/y.json", "kernel_sources_match": True,
                                             "measured_in_this_run": False},
          "find_neighbors": {"bound": "hbm", "ms": 0.061, "achieved": 675.0, "peak": 8000.0, "unit": "GB/s", "frac": 0.084},
          "find_neighbors_8rooms": {"bound": "hbm", "ms": 0.285, "achieved": 1160.0, "peak": 8000.0, "unit": "GB/s",
                                    "frac": 0.145, "rooms": 8, "points": 800000, "edges": 36000000,
                                    "algorithmic_bytes": 330000000}}
    layer = {"name": "Pool_0", "levels": [0, 1], "radius": 0.1, "fin": 1, "fout": 64, "fwd_ms": 0.083, "bwd_ms": 0.111,
             "roofline_fwd": dict(rl), "roofline_bwd": dict(rl), "note": "n" * 300}
    cfg = {"workload": "w" * 120, "points": 100000, "clouds": 1, "level_sizes": [100000, 5627, 1273, 318, 73],
           "convolutions": n_layers, "steps": 30, "ms_per_step": 4.9454, "value": 20220717.2, "unit": "points/s",
           "library_launches_per_step": 394.0, "host_issue_ms_per_step": 4.9373, "hierarchy_ms": 0.661,
           "mode": "pipelined+geometry", "host_lag_steps": 2, "sequential_ms_per_step": 6.8912, "host_busy_ms_per_step": 1.7421,
           "host_lag_wait_ms_per_step": 2.9811, "host_size_wait_ms_per_step": 0.2141, "bound_by": "gpu",
           "hierarchy_start": "after=True (batch resident in HBM)",
           "layers": [dict(layer) for _ in range(n_layers)],
           "cpu_baseline": {"value": 10437.1, "unit": "points/s", "cores": 128, "kind": "port", "sample": "s" * 300}}
    return {
        "metric": "MC-convolved points/sec (fwd+bwd), 100k-pt cloud r=0.1", "value": 172722645.0, "unit": "points/s",
        "n_gpus": 1, "steps": 100, "warmup": 10, "ms_per_step": 0.579, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "sequential": {"ms_per_step": 0.7005, "value": 142755174.9, "unit": "points/s"},
        "config": {"workload": "ScanNet-like non-uniform room " + "c" * 150, "points_total": 100000,
                   "points_per_gpu": 100000, "edges_per_gpu": 4543198, "layer": "1to64", "parallelism": "cloud-per-GPU dp1",
                   "headline_mode": "pipelined", "pipeline": "p" * 400, "pipelined_ms_per_step": 0.579,
                   "sequential_ms_per_step": 0.7005, "collective_backend": None, "rccl_world_size": 1,
                   "rank_stats": [{"rank": r, "ms": 0.6, "x": "y" * 50} for r in range(8)]},
        "roofline": rl,
        "cpu_baseline": {"value": 83697.6, "unit": "points/s", "cores": 128, "kind": "port", "host": "h" * 100,
                         "sample": "s" * 500, "single_thread": {"value": 9833.8, "unit": "points/s", "cores": 1,
                                                                "sample": "t" * 300}},
        "strong": {"rooms": 8, "points_total": 800000, "ms_per_step": 4.79, "value": 1.6e8, "unit": "points/s",
                   "scaling": "strong", "mode": "pipelined", "rank_stats": None, "note": "n" * 200},
        "layers": {n: {"ms_per_step": 1.0, "value": 1e8, "roofline": dict(rl), "conv_ms": {"fwd": 0.1, "bwd": 0.3},
                       "conv_rate": {"x": "y" * 300}} for n in ("1to64", "3to8", "dw256")},
        "configs": {"cfg%d" % i: dict(cfg) for i in range(5)},
        "breakdown": {"op%d" % i: {"ms": 0.1, "note": "b" * 100} for i in range(12)},
    }


def test_final_line_is_small_and_complete():
    b = _bench()
    rec = _full_record()
    assert len(json.dumps(rec)) > 30000  # the shape that broke the driver's parser
    line = b.compact_record(rec, "bench_details.json")
    assert len(line) < 4096 and "\n" not in line
    out = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in out, k
    assert out["value"] == rec["value"] and out["ms_per_step"] == rec["ms_per_step"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert out["roofline"][k] == rec["roofline"][k]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in out["cpu_baseline"]
    assert out["config"]["workload"] == rec["config"]["workload"] and "model" not in out["config"]
    assert out["strong"]["value"] == rec["strong"]["value"]
    # round-5 review, item 6: (a) the strictly sequential step at top level beside `value`; (b) numbers that come from a
    # committed profile are NAMED so and say whether the profile belongs to this tree's kernels; (c) the neighbour search
    # against the HBM roofline on one room AND on the 8-room batch
    assert out["sequential"] == rec["sequential"] and out["sequential"]["ms_per_step"] >= out["ms_per_step"]
    r = out["roofline"]
    assert "mfma_pipe_busy" not in r and "traffic_source" not in r
    assert r["mfma_pipe_busy_from_committed_profile"] == {"fwd": 0.31, "bwd": 0.24, "kernel_sources_match": True}
    assert r["traffic_from_committed_profile"] == {"bytes": 1224237649, "source": "profiles/y.json", "kernel_sources_match": True}
    for k in ("find_neighbors", "find_neighbors_8rooms"):
        assert r[k]["bound"] == "hbm" and r[k]["unit"] == "GB/s" and 0 < r[k]["frac"] < 1, k
    assert r["find_neighbors_8rooms"]["rooms"] == 8
    assert set(out["configs"]) == {"cfg0", "cfg1", "cfg2", "cfg3", "cfg4"}
    for c in out["configs"].values():
        assert {"ms_per_step", "value", "host_issue_ms_per_step", "launches", "host_busy_ms_per_step", "host_lag_wait_ms_per_step",
                "bound_by"} <= set(c)


def test_final_line_survives_errors_and_missing_objects():
    b = _bench()
    rec = _full_record()
    rec.update(roofline=None, cpu_baseline={"error": "x" * 5000}, strong=None, layers=None)
    rec["configs"] = {"cfg1": {"error": "e" * 5000}}
    out = json.loads(b.compact_record(rec))
    assert out["roofline"] is None and out["strong"] is None and len(out["configs"]["cfg1"]["error"]) <= 120


def test_emit_record_prints_the_compact_line_last(tmp_path, capsys):
    b = _bench()
    rec = _full_record()
    path = str(tmp_path / "d.json")
    b.emit_record(rec, path)
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 2 and lines[0].startswith("details: ") and len(lines[-1]) < 4096
    assert json.loads(lines[-1])["details"] == path
    assert json.load(open(path)) == rec == json.loads(lines[0][len("details: "):])


def test_profile_numbers_are_dropped_when_the_profile_is_of_other_sources(tmp_path):
    """bench.kernel_sources_sha1 == the hash tools/prof_summary.py records; a profile of other kernel sources does not
    supply the contract's `traffic`."""
    import subprocess
    import sys
    b = _bench()
    sha = b.kernel_sources_sha1()
    assert len(sha) == 40
    ps = os.path.join(ROOT, "tools", "prof_summary.py")
    code = "__file__ = %r; exec(open(__file__).read().split('SRC_SHA = _src_sha()')[0]); print(_src_sha())" % ps
    assert subprocess.check_output([sys.executable, "-c", code]).decode().strip() == sha


def test_last_committed_full_record_compacts():
    p = os.path.join(ROOT, "profiles", "r03_bench.json")
    rec = json.load(open(p))
    line = _bench().compact_record(rec, None)
    assert len(line) < 4096 and json.loads(line)["roofline"]["frac"] == rec["roofline"]["frac"]


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path):
    """--dump-outputs: float32 .npy files; above the byte limit the large arrays keep a seeded sample of their rows (the same
    rows in every run), the small ones are written whole."""
    import numpy as np
    b = _bench()
    rng = np.random.default_rng(0)
    arrs = {"conv_out": rng.random((100000, 8)), "features_grad": rng.random((100000, 1)).astype(np.float32),
            "Conv_weights_grad": rng.random((3, 64)).astype(np.float32)}
    limit = 2 ** 21
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), arrs, limit=limit)
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == ["Conv_weights_grad.npy", "conv_out.npy", "features_grad.npy"]
    loaded = {f: np.load(str(tmp_path / "a" / f)) for f in files}
    assert all(a.dtype == np.float32 for a in loaded.values())
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= limit + 1024
    assert np.array_equal(loaded["Conv_weights_grad.npy"], arrs["Conv_weights_grad"])
    assert 0 < loaded["conv_out.npy"].shape[0] < 100000 and loaded["conv_out.npy"].shape[1] == 8
    for f in files:
        assert np.array_equal(loaded[f], np.load(str(tmp_path / "b" / f))), f
    # below the limit everything is written whole
    b.dump_outputs(str(tmp_path / "c"), arrs)
    assert np.array_equal(np.load(str(tmp_path / "c" / "conv_out.npy")), arrs["conv_out"].astype(np.float32))
