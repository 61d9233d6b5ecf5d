"""bench.py's plain run and --dump-outputs: a plain run prints the headline line alone (what takes runs of its own is
behind --full) and --dump-outputs writes the state the last timed step left as float64 .npy files, cut to a fixed
sample when they would pass the size limit."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
NAMES = ("kf_q", "kf_t", "kf_vel", "cam_q", "cam_t", "chi2", "lm")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _FakeProblem:
    def __init__(self, n_kf, n_lm, n_cam):
        from amc_lba.abi import CAM_DTYPE, KF_DTYPE
        rng = np.random.default_rng(3)
        self.kfs = np.zeros(n_kf, KF_DTYPE)
        for f in ("q", "t", "vel"):
            self.kfs[f] = rng.standard_normal(self.kfs[f].shape)
        self.c = np.zeros(n_cam, CAM_DTYPE)
        self.c["q"], self.c["t"] = rng.standard_normal((n_cam, 4)), rng.standard_normal((n_cam, 3))
        self.lm = rng.standard_normal((n_lm, 3))

    def state(self):
        return self.kfs, self.lm

    def cams(self):
        return self.c


def test_dump_outputs_writes_the_state(tmp_path):
    b = _bench_module()
    p = _FakeProblem(7, 501, 4)
    st = types.SimpleNamespace(chi2_initial=3.0, chi2_final=2.0, lambda_final=0.5)
    b.dump_outputs(str(tmp_path / "o"), p, st, 0, 1)
    got = {n: np.load(tmp_path / "o" / f"{n}.npy") for n in NAMES}
    assert sorted(os.listdir(tmp_path / "o")) == sorted(n + ".npy" for n in NAMES)
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["kf_q"], p.kfs["q"]) and np.array_equal(got["kf_t"], p.kfs["t"])
    assert np.array_equal(got["kf_vel"], p.kfs["vel"]) and np.array_equal(got["lm"], p.lm)
    assert np.array_equal(got["cam_q"], p.c["q"]) and np.array_equal(got["cam_t"], p.c["t"])
    assert got["chi2"].tolist() == [3.0, 2.0, 0.5]


def test_dump_outputs_samples_past_the_limit(tmp_path, monkeypatch):
    b = _bench_module()
    p = _FakeProblem(7, 501, 4)
    st = types.SimpleNamespace(chi2_initial=3.0, chi2_final=2.0, lambda_final=0.5)
    small = sum(a.nbytes for a in (p.kfs["q"], p.kfs["t"], p.kfs["vel"], p.c["q"], p.c["t"])) + 24
    monkeypatch.setattr(b, "DUMP_BYTES", small + 100 * 24 + 5)   # room for 100 landmarks and a bit
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), p, st, 0, 1)
    la, lb = np.load(tmp_path / "a" / "lm.npy"), np.load(tmp_path / "b" / "lm.npy")
    assert la.shape == (100, 3) and np.array_equal(la, lb)   # the same rows every time
    rows = [int(np.flatnonzero((p.lm == r).all(1))[0]) for r in la]
    assert rows == sorted(set(rows))   # distinct rows of the state, in index order
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in os.listdir(tmp_path / "a")) <= b.DUMP_BYTES
    # several ranks share the limit and name their files apart
    b.dump_outputs(str(tmp_path / "r"), p, st, 1, 2)
    assert sorted(os.listdir(tmp_path / "r")) == sorted(f"rank1_{n}.npy" for n in NAMES)
    assert sum(np.load(tmp_path / "r" / f).nbytes for f in os.listdir(tmp_path / "r")) <= b.DUMP_BYTES // 2


@pytest.mark.gpu
def test_plain_run_line_and_outputs(tmp_path):
    """One small plain run: --steps sets the timed steps, the line carries the headline fields and none of --full's,
    and the dumped state is the window's (shapes) and finite."""
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "cfg0_cpu_plumbing", "--steps", "3",
                        "--warmup", "2", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["unit"] == "LM iterations/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-6 * 1e3   # one GPU: value is steps per second
    for k in ("roofline", "roofline_solve", "phases_ms_per_step", "localgpba_calls", "localgpba_map_calls",
              "cpu_baseline", "cpu_baseline_omp"):
        assert k not in d
    got = {n: np.load(out / f"{n}.npy") for n in NAMES}
    c = d["config"]
    assert got["kf_q"].shape == (c["n_kf"], 4) and got["kf_t"].shape == (c["n_kf"], 3)
    assert got["kf_vel"].shape == (c["n_kf"], 6) and got["lm"].shape == (c["n_lm"], 3)
    assert got["cam_q"].shape == (c["n_cam"], 4) and got["cam_t"].shape == (c["n_cam"], 3)
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert 0 < got["chi2"][1] <= got["chi2"][0]
