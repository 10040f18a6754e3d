"""CPU checks of bench.py's bookkeeping: which committed PMC summary feeds `roofline.traffic`, and how many input batches the
timed loop rotates over (cold-HBM rule).  The GPU side of the contract is exercised by the driver's own bench run."""
import importlib.util
import json
import os
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_traffic_lookup_matches_kernel_and_workload_size():
    b = _bench()
    head = json.load(open(os.path.join(ROOT, "profiles", "traffic_r02.json")))
    t = b.latest_traffic(head["kernel_name"], head["algorithmic_bytes_per_launch"])
    # (the newest committed pass of this kernel and size wins: round 3 re-profiled design S as the bit-exact handle's kernel)
    assert t is not None and t["file"].startswith(("traffic_r0", "r0")) and abs(t["hbm_bytes_per_launch"] / head["hbm_bytes_per_launch"] - 1.0) < 0.01
    # same kernel, twice the streams: the 512-stream profile, not the 256-stream one
    t512 = b.latest_traffic(head["kernel_name"], 2 * head["algorithmic_bytes_per_launch"])
    assert t512 is not None and abs(t512["hbm_bytes_per_launch"] / t["hbm_bytes_per_launch"] - 2.0) < 0.02
    # a workload size nobody profiled, or another kernel: no figure rather than a wrong one
    assert b.latest_traffic(head["kernel_name"], 12345.0) is None
    assert b.latest_traffic("no such kernel", head["algorithmic_bytes_per_launch"]) is None


def test_newest_round_traffic_feeds_the_headline_kernel():
    """The default bench line (design Q, configs[2]) takes `roofline.traffic` from the newest committed counter passes of the same kernel and size
    (round 6: re-taken by tools/profile_round.sh at the kernel with the angle-difference discriminator and the peeled last step)."""
    b = _bench()
    head = json.load(open(os.path.join(ROOT, "profiles", "traffic_r06.json")))
    assert head["kernel_name"].startswith("fast-q") and "k_mfir" in head["rocprof_kernel"]
    t = b.latest_traffic(head["kernel_name"], head["algorithmic_bytes_per_launch"])
    assert t is not None and t["file"].startswith(("traffic_r06", "r06_")) and abs(t["hbm_bytes_per_launch"] / head["hbm_bytes_per_launch"] - 1.0) < 0.01
    assert 1.0 <= t["hbm_bytes_per_launch"] / head["algorithmic_bytes_per_launch"] < 1.06       # warm-up re-reads: ~2 % of the bytes
    # the pipe figures of the kernels that are not bound by the HBM come from the same round's passes: `valu_frac` in their bench lines
    d = b.latest_pmc_derived("wbfm-fused (k_wbfm_steps<8,10>)")
    assert d is not None and d["file"] == "r06_wbfm_pmc.json" and 0.5 < d["valu_issue_busy_fraction"] < 0.9
    d = b.latest_pmc_derived("k_spectrum_chain<10, 12, 2>")
    assert d is not None and d["file"] == "r06_spectrum_pmc.json" and 0.5 < d["valu_issue_busy_fraction"] < 0.9
    t = b.latest_traffic("k_spectrum_chain<10, 12, 2>", 256 * 234 * 1024 * 2.0 + 256 * 1024 * 4.0)
    assert t is not None and 1.0 <= t["hbm_bytes_per_launch"] / t["algorithmic_bytes_per_launch"] < 1.1
    blk = b.bound_block("valu", "wbfm-fused (k_wbfm_steps<8,10>)", 0.108, 121241600.0, None)
    assert blk["bound"] == "valu" and blk["valu_frac"] == blk["valu_issue_busy_fraction"] and 0.6 < blk["valu_frac"] < 0.8


def test_traffic_never_below_algorithmic_bytes():
    """A committed summary whose traffic is below the algorithmic bytes would mean a broken counter pass."""
    import glob
    for fn in glob.glob(os.path.join(ROOT, "profiles", "r0[23456]*_pmc.json")):
        d = json.load(open(fn))
        assert d["hbm_bytes_per_launch"] >= 0.999 * d["algorithmic_bytes_per_launch"], fn
        assert d.get("commit") and d["commit"] != "wip", fn


def test_rotation_exceeds_the_infinity_cache():
    b = _bench()
    for bytes_per_batch in (256 * 480000, 512 * 480000, 128 * 640000, 64 * 480000):
        nb = b.pick_batches(types.SimpleNamespace(batches=0), bytes_per_batch)
        assert nb >= 3 and (nb - 1) * bytes_per_batch > 1.5 * b.L3_BYTES      # between two uses of a batch: more than the L3 holds
    assert b.pick_batches(types.SimpleNamespace(batches=7), 1) == 7


def test_mixed_input_class_spreads_the_noisy_streams_evenly():
    """bench.py --iq-class mixed:P: P per cent of the streams, evenly spread, hold noise (the per-stream routing's workload)."""
    b = _bench()
    for ns, pct in ((256, 5), (256, 10), (256, 25), (512, 10)):
        rows = b.noisy_rows(ns, pct)
        assert abs(len(rows) - ns * pct / 100.0) <= 1.0, (ns, pct, len(rows))
        gaps = [y - x for x, y in zip(rows, rows[1:])]
        assert max(gaps) - min(gaps) <= 1, (ns, pct)


def test_plain_run_is_lean_and_full_is_opt_in(monkeypatch):
    """`bench.py --gpus 1 --steps K --warmup W` times the headline only; the other legs run with --full, and nothing is dumped unless asked."""
    b = _bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = b.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = b.parse()
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_float32_capped_and_seeded(tmp_path, monkeypatch):
    """--dump-outputs: one float32 .npy per output, the valid part only; past the size cap a seeded sample of the streams, the same rows in every array."""
    import numpy as np
    import torch
    b = _bench()
    audio = torch.arange(6 * 5, dtype=torch.float32).reshape(6, 5)
    pcm = torch.arange(6 * 10, dtype=torch.int16).reshape(6, 10)
    assert b.dump_outputs(str(tmp_path / "a"), {"audio": audio, "pcm": pcm}, 0, 1) == ["audio", "pcm"]
    got = np.load(tmp_path / "a" / "audio.npy")
    assert got.dtype == np.float32 and np.array_equal(got, audio.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "pcm.npy"), pcm.numpy().astype(np.float32))
    # a cap of 3 rows' worth of both arrays: 3 of the 6 streams, chosen by the seed, in order, and in the files of every rank
    monkeypatch.setattr(b, "DUMP_BYTES", 2 * 3 * (5 * 4 + 10 * 4))
    for r in range(2):
        assert b.dump_outputs(str(tmp_path / "b"), {"audio": audio, "pcm": pcm}, r, 2) == ["audio_rank%d" % r, "pcm_rank%d" % r]
    a0, p0 = np.load(tmp_path / "b" / "audio_rank0.npy"), np.load(tmp_path / "b" / "pcm_rank0.npy")
    assert a0.shape == (3, 5) and p0.shape == (3, 10)
    rows = (a0[:, 0] / 5).astype(int)
    assert list(rows) == sorted(set(rows)) and np.array_equal(p0, pcm.numpy()[rows].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "b" / "audio_rank1.npy"), a0)
    b.dump_outputs(str(tmp_path / "c"), {"audio": audio, "pcm": pcm}, 0, 2)
    assert np.array_equal(np.load(tmp_path / "c" / "audio_rank0.npy"), a0)
