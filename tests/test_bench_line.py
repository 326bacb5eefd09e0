"""bench.py's printed line (CPU): compact, parseable, contract keys first.

Round 3's line grew to ~21 KB and the driver, which keeps a bounded tail of
stdout, could not parse it. compact_line() must keep the line
under LINE_MAX_BYTES on a recorded full result and keep the keys the driver
and the judge read; --gpus must never silently run one GPU.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

RECORDED = os.path.join(ROOT, "profiles", "r03", "final3", "bench.json")
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def _recorded():
    with open(RECORDED) as f:
        return json.load(f)


def test_compact_line_of_recorded_result_fits_and_keeps_keys():
    full = _recorded()
    assert len(json.dumps(full)) > 16000  # the round-3 line that the driver could not parse
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    s = json.dumps(line)
    assert len(s) <= bench.LINE_MAX_BYTES
    assert len(s) <= 4096
    assert list(line)[:len(CONTRACT)] == list(CONTRACT)
    assert json.loads(s) == line
    assert line["value"] == pytest.approx(full["value"], rel=1e-5)
    assert line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"]
    assert line["roofline"]["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-3)
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"]
    assert line["config"]["workload"].startswith("config2")
    assert line["digest_match"] is True
    # every config of BASELINE.json has its sub-object
    cfg = line["configs"]
    for k in ("c1_paillier", "c2_per_op_2048", "c3_safe_primes", "c4_sign", "c4_sign_3_signers", "c5_keygen"):
        assert k in cfg, k
        assert cfg[k]["value"] > 0
    assert cfg["c4_sign"]["cpu"] == pytest.approx(full["signing"]["cpu_baseline"]["value"], rel=1e-3)
    assert line["detail"] == "gpurun_out/bench_detail.json"


def test_compact_line_never_exceeds_limit():
    full = _recorded()
    full["signing"]["unit"] = "x" * 5000  # pathological sub-line
    line = bench.compact_line(full, "d.json")
    assert len(json.dumps(line)) <= bench.LINE_MAX_BYTES
    assert line["value"] == pytest.approx(full["value"], rel=1e-5)


def test_config1_value_is_single_batch_and_in_flight_is_labelled():
    """BASELINE configs[0] is ONE batch of 1,024 ops: c1_paillier.value is that
    rate; the concurrent-batches rate is a second, labelled key (VERDICT r4
    item 4)."""
    full = _recorded()
    full["paillier_batch"] = {
        "value": 40000.0, "unit": "Encrypt+HomoMult ops/s", "n_gpus": 1,
        "roofline": {"frac": 0.11}, "cpu_baseline": {"value": 550.0, "cores": 16},
        "batches_in_flight": {"batches": 16, "value": 88000.0, "seconds": 3.7}}
    line = bench.compact_line(full, "d.json")
    c1 = line["configs"]["c1_paillier"]
    assert c1["value"] == pytest.approx(40000.0)
    assert c1["batches_in_flight"] == 16
    assert c1["in_flight_value"] == pytest.approx(88000.0)
    assert c1["frac"] == pytest.approx(0.11)
    assert len(json.dumps(line)) <= bench.LINE_MAX_BYTES


def test_world_size_mismatch_exits_nonzero():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr
    assert r.stdout == ""


def test_gpus_without_launcher_relaunches_under_torchrun(monkeypatch):
    calls = []

    def fake_call(cmd):
        calls.append(cmd)
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    (cmd,) = calls
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"]


def test_dump_rows_fixed_sample_within_size_bound():
    """--dump-outputs: every operand of a small batch, a fixed ascending sample of
    a batch whose float64 words would pass DUMP_MAX_BYTES (the bench's 65,536 x
    128 words is exactly twice the bound), the same rows on every call."""
    import numpy as np
    assert list(bench.dump_rows(5, 128)) == [0, 1, 2, 3, 4]
    keep = bench.DUMP_MAX_BYTES // (8 * 128)
    assert list(bench.dump_rows(keep, 128)) == list(range(keep))
    rows = bench.dump_rows(65536, 128)
    assert len(rows) == keep == 32768 and rows.dtype == np.int64
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 65536
    assert np.array_equal(rows, bench.dump_rows(65536, 128))
    assert len(bench.dump_rows(keep + 1, 128)) == keep


def test_dump_outputs_writes_exact_float64_words(tmp_path):
    import numpy as np
    out = np.array([[0, 1, 0xFFFFFFFF], [0x80000000, 0x12345678, 7]], dtype=np.uint32)
    d = tmp_path / "dump" / "nested"
    bench.dump_outputs(str(d), "modexp_out", out.view(np.int32))  # the device tensor's dtype is int32
    got = np.load(d / "modexp_out.npy")
    assert got.dtype == np.float64 and got.shape == (2, 3)
    assert np.array_equal(got.astype(np.uint64), out.astype(np.uint64))
    assert np.array_equal(np.load(d / "modexp_out_rows.npy"), np.array([0.0, 1.0]))
    assert sorted(p.name for p in d.iterdir()) == ["modexp_out.npy", "modexp_out_rows.npy"]


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "--steps" in str(e.value.code)


def test_mx_executed_floor_counts_the_schedule():
    """bench.mx_floor: the executed-work floor of k_modexp_mx counts
    the sliding-window schedule of the exponent and prices the product loops' MADs
    and the reduction's i8 MACs at their peaks."""
    import bench
    # 0b1011 with width 6: one window (the top), no squarings after it
    assert bench.sliding_window_counts(0b1011) == (0, 6, 0)
    # 2^10 + 1: top window 1, then 10 squarings and one window multiply
    sq, tab, wins = bench.sliding_window_counts((1 << 10) + 1)
    assert (sq, wins) == (10, 1) and tab == 1
    f = bench.mx_floor(65536, (1 << 2047) | 1, 100.0)
    assert f["squarings"] == 2048 and f["products"] >= 2
    assert abs(f["valu_lane_mads"] - 65536 * (2048 * 148 * 19 * 4 + f["products"] * 148 * 37 * 4)) < 1
    assert f["floor_ms_valu"] > f["floor_ms_mfma"] > 0
    assert abs(f["frac_of_floor"] - f["floor_ms_valu"] / 100.0) < 1e-9


def test_two_pipe_roofline_is_a_utilisation():
    """k_modexp_mx (VALU product loop + i8 matrix-core reduction): the printed
    roofline's frac is the executed-work floor's (<= 1), bound names both pipes,
    and the Go-equivalent INT32 ratio and the i8 peak sit under their own keys
    (VERDICT r5 item 3). Replayed on round 5's recorded driver-shaped result."""
    import copy
    with open(os.path.join(ROOT, "profiles", "r05", "final5", "bench_detail.json")) as f:
        full = json.load(f)
    r0 = copy.deepcopy(full["roofline"])
    assert r0["kernel"] == "k_modexp_mx" and r0["frac"] > 0.95  # the old definition, near / above 1 at clock
    bench.two_pipe_roofline(full["roofline"])
    r = full["roofline"]
    assert r["bound"] == "valu+mfma_i8" and r["binding_pipe"] == "valu"
    assert r["frac"] == pytest.approx(r0["executed_floor"]["frac_of_floor"], rel=1e-9)
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-9)
    assert 0 < r["frac"] <= 1 and 0 < r["frac_i8"] <= 1 and r["frac_at_clock"] <= 1
    assert r["go_equiv_frac"] == pytest.approx(r0["frac"]) and r["go_equiv_frac_at_clock"] > 1
    assert r["peak_i8"] == pytest.approx(bench.PEAK_I8_MFMA / 1e12)
    line = bench.compact_line(full, "d.json")
    lr = line["roofline"]
    assert lr["kernel"] == "k_modexp_mx" and lr["frac"] <= 1
    for k in ("go_equiv_frac", "peak_i8", "peak", "binding_pipe", "frac_i8"):
        assert k in lr, k
    assert len(json.dumps(line)) <= bench.LINE_MAX_BYTES
