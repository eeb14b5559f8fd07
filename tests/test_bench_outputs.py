"""bench.py's options for a plain run and --dump-outputs, on CPU: a run without --full measures the
metric alone, --steps is at least one, and the dump writes float64 / float32 arrays within 64 MB in
all, a larger output as the same seeded sample of its elements in every run."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_a_plain_run_leaves_the_legs_beside_the_metric_out():
    a = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.steps == 5 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


@pytest.mark.parametrize("bad", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_and_warmup_are_checked(bad):
    with pytest.raises(SystemExit):
        bench.parse_args(bad)


def _size(d):
    return sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d))


def test_dump_writes_the_frame_in_full_and_a_seeded_sample_of_the_display_bytes(tmp_path):
    h, w = 1080, 1920
    frame = torch.arange(h * w * 3, dtype=torch.float64).reshape(h, w, 3) / 7.
    display = (torch.arange(h * w * 3) % 251).to(torch.uint8).reshape(h, w, 3)
    info = bench.dump_outputs(str(tmp_path / "a"), {"frame": frame, "display": display})
    f, g = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "display.npy")
    assert f.dtype == np.float64 and np.array_equal(f, frame.numpy())
    assert g.dtype == np.float32 and g.shape == (3_000_000,)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(h * w * 3, 3_000_000, replace=False))
    assert np.array_equal(g, display.numpy().reshape(-1)[idx].astype(np.float32))
    assert info["frame"] == {"shape": [h, w, 3], "dtype": "float64", "sample": None}
    assert info["display"]["shape"] == [h, w, 3] and info["display"]["sample"].startswith("3000000 of 6220800")
    assert _size(tmp_path / "a") <= 64 * 10 ** 6
    bench.dump_outputs(str(tmp_path / "b"), {"frame": frame, "display": display})
    for n in ("frame.npy", "display.npy"):
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes()


def test_a_frame_larger_than_its_share_is_sampled(tmp_path):
    frame = torch.linspace(0., 1., 1200 * 1920 * 3, dtype=torch.float64).reshape(1200, 1920, 3)
    info = bench.dump_outputs(str(tmp_path), {"frame": frame})
    f = np.load(tmp_path / "frame.npy")
    assert f.dtype == np.float64 and f.shape == (6_250_000,) and info["frame"]["sample"]
    assert np.all(np.diff(f) > 0)                                 # sorted positions of a rising ramp
    assert _size(tmp_path) <= 64 * 10 ** 6
