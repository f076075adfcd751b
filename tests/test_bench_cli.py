"""bench.py's command line and its --dump-outputs writer, on CPU: what a plain run times, which options need --full, and the files a
dump leaves (names, dtypes, the 64 MB budget, the seeded sample of an output larger than its share)."""
import os

import numpy as np
import torch

import bench


def test_plain_run_times_exactly_steps():
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not args.full and args.dump_outputs is None and args.blocks == 1
    calls = []
    times = bench.timed_blocks(lambda i: calls.append(i), lambda: None, None, bench.NoDist(), lambda: None, args.steps, args.warmup, args.blocks)
    assert len(times) == 1 and calls == list(range(9))              # 2 warm-up steps, then ONE block of exactly 7 timed steps


def test_full_and_profile_json():
    assert bench.parse_args(["--full"]).full
    assert bench.parse_args(["--profile-json", "p.json"]).full      # the per-kernel table comes from the profiled frame
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"


def _outs():
    g = torch.Generator().manual_seed(0)
    return {"bbox_map": torch.rand(2, 256, 4, generator=g), "search": torch.rand(2, 256, 96, generator=g),
            "argmax": torch.tensor([3, 250], dtype=torch.int64), "flag": torch.tensor([2, 2]), "prompt": torch.zeros(2, 3, 96),
            "prompts": torch.zeros(2, 3, 96)}


def test_dump_outputs_in_full(tmp_path):
    outs = _outs()
    written = bench.dump_outputs(outs, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["argmax.npy", "bbox_map.npy", "search.npy"]        # the echoed inputs are not outputs
    for k in ("bbox_map", "search"):
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == np.float32 and written[k] == (tuple(outs[k].shape), outs[k].numel())
        np.testing.assert_array_equal(a, outs[k].numpy())
    a = np.load(tmp_path / "argmax.npy")
    assert a.dtype == np.float64 and a.tolist() == [3.0, 250.0]


def test_dump_outputs_samples_what_exceeds_the_budget(tmp_path):
    outs = _outs()
    budget = 40000                                                  # search (196 KB) does not fit; argmax and bbox_map (8 KB) do
    w1 = bench.dump_outputs(outs, str(tmp_path / "a"), budget=budget)
    w2 = bench.dump_outputs(outs, str(tmp_path / "b"), budget=budget)
    assert w1 == w2
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))        # (128-byte .npy headers)
    assert total <= budget
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "bbox_map.npy"), outs["bbox_map"].numpy())
    s1, s2 = np.load(tmp_path / "a" / "search.npy"), np.load(tmp_path / "b" / "search.npy")
    assert s1.ndim == 1 and 0 < s1.size < outs["search"].numel() and s1.size == w1["search"][1]
    np.testing.assert_array_equal(s1, s2)                           # the same elements every time
    assert np.isin(s1, outs["search"].numpy().reshape(-1)).all()
