"""bench.py's options on the CPU: a plain run times the headline only (everything else is behind --full), --steps is a
positive count, and --dump-outputs writes float32 / float64 arrays bit for bit, sampled by a fixed seed under 64 MB."""
import os

import numpy as np
import pytest

import bench
from conftest import same_f32

OFF_IN_A_PLAIN_RUN = ("no_cpu_baseline", "no_alt", "no_extra", "no_verify")


def test_plain_run_is_the_headline_only():
    a = bench.parse_args(["--steps", "7", "--warmup", "3"])
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 3)
    assert all(getattr(a, k) for k in OFF_IN_A_PLAIN_RUN)


def test_full_runs_every_block_unless_left_out():
    a = bench.parse_args(["--full"])
    assert a.full and not any(getattr(a, k) for k in OFF_IN_A_PLAIN_RUN)
    a = bench.parse_args(["--full", "--no-verify", "--dump-outputs", "d"])
    assert a.no_verify and not a.no_alt and a.dump_outputs == "d"


@pytest.mark.parametrize("steps", ["0", "-2"])
def test_steps_must_be_positive(steps):
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", steps])


def _records(planes, n, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((planes, n)).astype(np.float32)
    a[0, :3] = [np.nan, -0.0, np.inf]
    return {"idx_local": rng.integers(0, 1 << 24, (planes, n)).astype(np.int32), "a": a,
            "b": rng.standard_normal((planes, n)).astype(np.float32), "iso": rng.integers(0, 8, (planes, n)).astype(np.int32),
            "qrows": rng.integers(-1 << 20, 1 << 20, (planes, n, 3)).astype(np.int32)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_whole(tmp_path):
    res = _records(3, 500)
    names = bench.dump_outputs(str(tmp_path), res)
    got = _load(str(tmp_path))
    assert names == sorted(res) == sorted(got)
    for k, v in res.items():
        assert got[k].shape == v.shape
        if v.dtype == np.float32:
            assert got[k].dtype == np.float32 and same_f32(got[k], v), k
        else:
            assert got[k].dtype == np.float64 and (got[k] == v).all(), k


def test_dump_outputs_without_plane_dimension(tmp_path):
    res = {k: v[0] for k, v in _records(1, 400).items()}          # --inproc: [N] and [N, 3]
    bench.dump_outputs(str(tmp_path), res)
    got = _load(str(tmp_path))
    assert got["qrows"].shape == (400, 3) and (got["qrows"] == res["qrows"]).all() and same_f32(got["a"], res["a"])


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    res = _records(4, 3000)
    limit = 60000
    d1, d2 = str(tmp_path / "1"), str(tmp_path / "2")
    bench.dump_outputs(d1, res, limit_bytes=limit)
    bench.dump_outputs(d2, res, limit_bytes=limit)
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1)) <= limit
    g1, g2 = _load(d1), _load(d2)
    assert sorted(g1) == sorted(res) + ["sample_index"]
    pick = g1["sample_index"].astype(np.int64)
    assert (pick == g2["sample_index"]).all() and len(pick) > 100 and (np.diff(pick) > 0).all()
    for k, v in res.items():
        flat = v.reshape((-1,) + v.shape[2:])[pick]
        assert same_f32(g1[k], flat) if v.dtype == np.float32 else (g1[k] == flat).all(), k
