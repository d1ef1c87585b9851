"""CPU: bench.py's result check (the comparison of a step's result with the committed digests of the reference objects' result,
tests/golden/fullsize_*.json) - the logic alone, on made-up digests; the GPU suite runs it on real results (test_gpu_bench.py)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _inputs(want, with_sens=False):
    import bench

    stages = bench.RESULT_STAGES_SENS if with_sens else bench.RESULT_STAGES
    first = {k: want[k] for k in stages if k in want and not k.startswith(("valid", "rows"))}
    return first


def test_result_check_against_a_committed_file(tmp_path, monkeypatch):
    import bench

    want = json.load(open(os.path.join(ROOT, "tests", "golden", "fullsize_c2.json")))
    assert want["backend"] == "reference-objects"
    for k in ("rows0", "rows0_sum", "rows2", "rows2_sum"):
        assert k in want, "tests/golden/fullsize_c2.json lacks the digest of every pile row (%s)" % k
    first = _inputs(want)
    valid = np.zeros(16, dtype=np.uint8)
    rows = np.zeros(4, dtype=np.uint64)
    # the replicated stages equal, the made-up validity bytes and row checksums not: the check fails and says where
    out, ok = bench.result_check("c2", False, first, dict(first), valid, rows, rows, [0, 7])
    assert not ok and out["ok"] is False and out["ranks_agree"]
    assert set(out["stages_differ"]) == {"valid", "rows2", "rows2_sum"}
    assert set(out["stages_equal"]) == set(first)
    assert out["digests"] == "tests/golden/fullsize_c2.json" and out["ranks_checked"] == [0, 7]
    # two ranks that disagree fail whatever the file says
    last = dict(first, edges="0" * 64)
    out, ok = bench.result_check("c2", False, first, last, valid, rows, rows, [0, 1])
    assert not ok and not out["ranks_agree"]
    # a workload without a digest file: nothing to compare with, agreement of the ranks is all there is
    out, ok = bench.result_check("c5", False, first, dict(first), valid, rows, rows, [0, 7])
    assert ok and out["ok"] is None and out["digests"] is None and out["ranks_agree"]
    out, ok = bench.result_check("c5", False, first, last, valid, rows, rows, [0, 7])
    assert not ok and out["ok"] is False


def test_result_check_passes_on_the_committed_digests(monkeypatch):
    """every stage as the file has it: ok (the validity / row digests injected through the digest function)"""
    import bench

    want = json.load(open(os.path.join(ROOT, "tests", "golden", "fullsize_c3.json")))
    first = _inputs(want)
    answers = iter([want["valid"], want["rows2"], want["rows2_sum"]])
    monkeypatch.setattr(bench, "_dg", lambda *a: next(answers))
    out, ok = bench.result_check("c3", False, first, dict(first), np.zeros(8, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint64), [0, 7])
    assert ok and out["ok"] is True and not out["stages_differ"] and len(out["stages_equal"]) == len(bench.RESULT_STAGES)


def test_dump_outputs_stays_within_its_budget(tmp_path):
    """bench.dump_outputs: float32 where exact, float64 otherwise; an array beyond its share of the budget keeps a seeded sample
    of its entries, the same in every run; the files together stay under 64 MB"""
    import bench

    arrays = {"valid": (np.arange(40_000_000) % 3 == 0).astype(np.uint8), "small": np.arange(1000, dtype=np.uint32),
              "wide": np.arange(3_000_000, dtype=np.uint64) << np.uint64(30), "one": np.array([7], dtype=np.uint64)}
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), arrays)
    names = sorted(os.listdir(tmp_path / "0"))
    assert names == ["lengths.npy", "one.npy", "small.npy", "valid.npy", "wide.npy"]
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in names) <= 64 << 20
    got = {f: np.load(tmp_path / "0" / f) for f in names}
    for f in names:
        assert np.array_equal(got[f], np.load(tmp_path / "1" / f)), f
    assert got["small.npy"].dtype == np.float32 and np.array_equal(got["small.npy"], np.arange(1000))
    assert got["wide.npy"].dtype == np.float64 and 0 < len(got["wide.npy"]) < 3_000_000
    assert np.all(np.fmod(got["wide.npy"], float(1 << 30)) == 0)          # sampled entries, exact
    assert got["valid.npy"].dtype == np.float32 and 0 < len(got["valid.npy"]) < 40_000_000
    assert list(got["lengths.npy"]) == [1, 1000, 40_000_000, 3_000_000]
