"""CPU: bench.py's command line (a plain run measures the headline mode only; --full adds the other measurements) and the
--dump-outputs writer."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_cli", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_measures_the_headline_only_and_full_restores_the_rest(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.also == "none" and a.no_prof and a.no_parity_check and a.no_cpu_baseline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.also == "f32,f16"
    assert not (a.no_prof or a.no_parity_check or a.no_cpu_baseline)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--also", "none", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.also == "none" and a.no_cpu_baseline and not a.no_prof


def test_write_outputs_as_float_arrays(tmp_path):
    bench = _bench()
    m = {"map_sample": np.linspace(0, 1, 10, dtype=np.float32), "rects": np.array([[0, 1, 2, 3, 4], [1, 5, 6, 7, 8]], np.int32),
         "counts": [1, 1, 0], "texts": ["ab", "Việt"]}
    bench.write_outputs(str(tmp_path / "out"), m)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == ["boxes_per_page", "det_map_sample", "rects", "texts"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["det_map_sample"], m["map_sample"])
    assert np.array_equal(got["rects"], m["rects"]) and np.array_equal(got["boxes_per_page"], [1, 1, 0])
    assert got["texts"].shape == (2, 4)
    assert ["".join(chr(int(c)) for c in row if c >= 0) for row in got["texts"]] == m["texts"]
    # a workload without maps or strings (--boxes synthetic-gt, --workload det) writes what it has
    bench.write_outputs(str(tmp_path / "det"), {"map_sample": None, "rects": m["rects"], "counts": [], "texts": None})
    assert os.listdir(tmp_path / "det") == ["rects.npy"]
