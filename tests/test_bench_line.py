"""bench.py's LAST stdout line must stay a compact JSON record (< 4 KB) carrying the headline, `roofline` and
`cpu_baseline`: round 2's line outgrew the driver's tail and its record did not parse."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _canned_record(bench, name, prose=4000):
    note = "x" * prose            # the full records carry long prose notes: none of it may reach the last line
    return {"metric": "aggregate-verify signer-pairs/sec", "value": 14234567.891, "unit": "signer-pairs/s", "ms_per_step": 73.66612345, "ms_per_step_min": 72.1,
            "ms_per_step_all": [72.1, 73.7, 74.9], "steps": 20, "warmup": 5, "repetitions": 3, "n_gpus": 1, "dtype": "u32", "data": "synthetic",
            "config": {"workload": note, "curve": name, "signers": 1 << 20, "signers_per_gpu": 1 << 20, "in_flight": 4, "parallelism": note},
            "roofline": {"bound": "valu-int32-mac", "kernel": "k_miller_s60<BN254>", "peak": 33.251234, "unit": "TMAC/s", "achieved": 15.9, "frac": 0.4781234,
                         "launch_ms": 4.6, "launches_per_step": 16, "macs_per_launch": 7.35e10, "traffic": 104857600,
                         "traffic_detail": {"note": note, "valu_busy": 0.8191234, "lds_conflict_ratio": 0.1021234, "kernel_clock_ghz": 2.3426,
                                            "counters_from": "profiles/r6 (builder run)"},
                         "exclusive": {"kernel": "k_miller_ab64<BN254>", "launch_ms": 5.788, "achieved": 12.7, "frac": 0.3912345, "note": note},
                         "hbm_side": {"achieved": 2.7, "peak": 8000.0, "unit": "GB/s", "note": note}, "whole_path_frac": 0.52, "note": note},
            "sequential": {"ms_per_step_median": 91.0, "note": note}, "stage_ms_per_step": {"miller": 70.0}, "stage_ms_exclusive": {"miller": 84.0},
            "cpu_baseline": {"value": 8912.3, "unit": "signer-pairs/s", "cores": 192, "host_cores": 192, "kind": "port", "per_core_ms_per_pairing": 2.61, "sample": note}}


def test_last_line_is_compact_and_complete():
    bench = _bench()
    full = _canned_record(bench, "altbn128")
    bench.cycle_roofline(full["roofline"])
    full.update({"higher_is_better": True, "scaling": "strong", "vs_baseline": None})
    full["records"] = {k: _canned_record(bench, "bls12") for k in
                       ("bls12_1048576", "altbn128_65536", "bls12_65536", "altbn128_1048576_prepared_keys", "bls12_1048576_prepared_keys",
                        "altbn128_multisig_1048576", "altbn128_multisig_batch_64x16384", "altbn128_64")}
    full["collective"] = {"backend": "nccl", "world": 8, "rccl_version": "2.22.3", "bytes_per_step": 8 * 580, "op": "all_gather"}
    line = bench.compact_line(full)
    assert len(line) < 4096, len(line)
    assert "\n" not in line
    rec = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline", "records"):
        assert key in rec, key
    assert rec["config"]["curve"] == "altbn128" and rec["config"]["signers"] == 1 << 20
    roof = rec["roofline"]
    # frac = the exclusive, rocprof-reproducible figure; the timed-region reading is labelled
    assert roof["kernel"] == "k_miller_ab64<BN254>" and abs(roof["frac"] - 0.3912) < 1e-3
    assert abs(roof["frac_timed_region"] - 0.4781) < 1e-3 and roof["kernel_timed_region"] == "k_miller_s60<BN254>"
    assert set(roof) >= {"bound", "kernel", "peak", "achieved", "frac", "launch_ms", "traffic", "unit"}
    # north_star: "evidenced by rocprof HBM GB/s and VALU-busy against gfx950 peak" -- the evidence run's counter readings ride along
    assert abs(roof["valu_busy"] - 0.8191) < 1e-3 and abs(roof["lds_conflict_ratio"] - 0.1021) < 1e-3 and roof["hbm_gbps"] == 2.7
    # the cycle-basis reading beside `frac`, and the label saying the counters are the evidence run's
    pk = 16 * 1024 * 2.3426e9 / 1e12
    assert abs(roof["peak_at_kernel_clock"] - pk) < 0.02 and abs(roof["kernel_clock_ghz"] - 2.343) < 1e-3
    assert abs(roof["frac_cycles"] - 12.7 / pk) < 1e-3 and roof["frac_cycles"] < roof["frac"]
    assert roof["counters_from"] == "profiles/r6 (builder run)"
    # every host core the oracle can use, not a cap of 64
    assert rec["cpu_baseline"]["cores"] == 192 and rec["cpu_baseline"]["host_cores"] == 192
    assert rec["cpu_baseline"]["kind"] == "port" and len(rec["cpu_baseline"]["sample"]) <= 120
    assert len(rec["records"]) == 8
    for r in rec["records"].values():
        assert set(r) <= {"value", "ms_per_step", "frac", "cpu", "cpu_cores"}
    # config 1 carries a CPU figure at its own shape (n = 64, all cores): the canned altbn128_64 record has one
    assert rec["records"]["altbn128_64"]["cpu"] == 8912.0 and rec["records"]["altbn128_64"]["cpu_cores"] == 192


def test_cpu_baseline_is_not_capped_at_64_threads(monkeypatch):
    """cpu_baseline() capped its threads at 64 although SURVEY 8d says 'all host cores, count printed' and the oracle
    takes 256.  Source rule + the helper's own arithmetic on a faked 192-core host."""
    import inspect
    bench = _bench()
    src = inspect.getsource(bench.cpu_baseline)
    assert "min(cores, 64)" not in src and "min(cores, 256)" in src
    src_small = inspect.getsource(bench.cpu_baseline_small)
    assert "sched_getaffinity" in src_small and "verify_aggregate" in src_small and "min(cores, n + 1)" in src_small


def test_plain_run_line_is_complete():
    """A run without --full has no roofline, CPU baseline or other records: its line carries the headline and those three empty."""
    bench = _bench()
    full = _canned_record(bench, "altbn128")
    full.pop("cpu_baseline")
    full.update({"roofline": None, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "records": {}})
    rec = json.loads(bench.compact_line(full))
    assert rec["value"] == 14234600.0 and rec["ms_per_step"] == 73.6661 and rec["unit"] == "signer-pairs/s" and rec["dtype"] == "u32"
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["records"] == {}


def test_line_shrinks_rather_than_overflowing():
    bench = _bench()
    full = _canned_record(bench, "altbn128")
    full["records"] = {"record_with_a_long_name_%03d" % i: _canned_record(bench, "bls12", 10) for i in range(120)}
    line = bench.compact_line(full)
    assert len(line) < 4096 and json.loads(line)["value"] > 0
    full["records"] = {"r%d" % i: _canned_record(bench, "bls12", 10) for i in range(40)}
    assert len(bench.compact_line(full)) < 4096


def test_dump_outputs_writes_float_arrays(tmp_path):
    """--dump-outputs: one DIR/<name>.npy per array, float32 / float64 only, and nothing over 64 MB in all."""
    import numpy as np
    import pytest
    bench = _bench()
    arrays = {"verdict": np.array([1.0]), "gt_partial": np.arange(384, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    for k, v in arrays.items():
        got = np.load(str(tmp_path / "d" / (k + ".npy")))
        assert got.dtype == v.dtype and np.array_equal(got, v)
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "e"), {"raw": np.zeros(4, dtype=np.uint8)})
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "f"), {"big": np.zeros((64 << 20) // 8 + 1, dtype=np.float64)})


def test_stage_time_is_per_call_not_per_scope():
    """the key-sum stage of a multi-signature check was divided by the stage's scope COUNT (two scopes per check), which
    halved it.  The per-call figure must equal the rocprof-style sum of the stage's kernels whatever the number of scopes."""
    import pytest
    bench = _bench()
    # rocprof summary of one check (profiles/r3/stats_multisig_1048576): main pass, 12 tree levels, conversion
    kernels_ms = [0.680] + [0.243 / 12] * 12 + [0.117]
    calls = 5
    total_ms = sum(kernels_ms) * calls
    for scopes_per_call in (1, 2, 3):
        count = scopes_per_call * calls                                   # what bgls_profile_get reports as `launches`
        assert abs(bench.stage_ms_per_call(total_ms, calls) - sum(kernels_ms)) < 1e-9, count
        if scopes_per_call > 1:
            assert total_ms / count < 0.6 * sum(kernels_ms)               # the old arithmetic, for the record
    with pytest.raises(ValueError):
        bench.stage_ms_per_call(1.0, 0)
