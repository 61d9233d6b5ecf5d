"""The lane maps of k_lin_schur's per-tile phases at the tile shapes where they can go wrong.

Phase 2 (pose-sample partials M / g) runs one lane per (tile sample, group of three outputs), phase 4 (Hll / bl)
one lane per landmark over an unrolled row loop, phase 6 (S partials) splits a last pass of at most half the
workgroup over lane pairs that swap their blocks before the store, and phase 7 (rhs partials) counts its tasks
from the top lane.  Each window below is the smallest that forces one edge of those maps; each is compared with the CPU oracle at tests/test_gpu_parity.py's tolerances
(fp32-residual case: tests/test_gpu_f32_residual.py's): lba_linearize (residuals, H_pp, b, H_ll), solve_step at
lambda = 1 and 1e-3, optimize(10) with the oracle's trial count.

  full_lm_tile   every landmark has exactly two non-GP mono observations: tiles fill to TILE_LMS = 64 landmarks
                 (phase 4 on every lane of the top wave, 128 observations, 256 rows, 9 samples of up to 104 rows)
  long_sample    two free keyframes and a fixed one, non-GP stereo observations only: at most three samples
                 per tile, one of them with >= 150 of the tile's <= TILE_ROWS = 288 rows (a long row loop next
                 to short ones)
  many_samples   GP observations each at its own time stamp (2-row and 3-row): a tile approaches TILE_SMP = 64
                 samples of one row group each (phase 2 takes more than two passes)
  minimal        one stereo observation of one landmark (two free keyframes, one of them unobserved): one tile,
                 one sample, one pair, one Schur entry (every pass is ragged; phase 6 is one split pass of 8 tasks)
  mixed_rows     LBA_STEREO_GP and LBA_MONO_GP observations interleaved in a tile (2- and 3-row groups)
  heavy          landmarks seen from more keyframes than a tile holds: segment tiles, which stop after phase 3
  schur_36       8 free keyframes: tiles with 33..40 Schur entries (phase 6: one full pass and a split pass of
                 <= 64 tasks, phase 7 on the lanes above it)
  schur_66       12 free keyframes: 65..80 entries (two full passes, then a split pass)
  (mixed_rows again with LBA_FLAG_F32_RESIDUAL: the <true> instantiation)

The CPU test asserts with lba_setup_tile_shapes (the host tiling, no device) that every window has the shape
it is named for.
"""
import functools
from dataclasses import replace

import numpy as np
import pytest

import amc_lba
import orc
import window_mutations as wm
from amc_lba import Problem
from amc_lba.abi import FLAG_F32_RESIDUAL, MONO, STEREO
from amc_lba.synth import make_window
from test_heavy_landmarks import _spanning

TILE_LMS, TILE_SMP, TILE_ROWS, TILE_OBS = 64, 64, 288, 128


def _remeasure(win, obs, seed):
    """The window with the observations `obs`, every measurement the oracle's projection at the window's estimate
    plus one pixel of noise (float32 like every stored measurement); observations a tracker could not have made
    (depth test, outside the 960 x 600 image) and landmarks left without one are dropped."""
    rng = np.random.default_rng(seed)
    obs = obs.copy()
    obs["z"] = 0.0
    o = orc.Oracle(replace(win, obs=obs))
    _, res, _ = o.errors()
    z = -res + rng.normal(0, 1.0, res.shape)
    st = (obs["kind"] == STEREO) | (obs["kind"] == wm.STEREO_GP)
    z[~st, 2] = 0.0
    keep = o.depth_ok().astype(bool) & (z[:, 0] >= 0) & (z[:, 0] < wm.IMG_W) & (z[:, 1] >= 0) & (z[:, 1] < wm.IMG_H)
    obs["z"] = wm._f32(z)
    obs = obs[keep]
    seen = np.unique(obs["lm"])
    remap = -np.ones(len(win.lm), np.int64)
    remap[seen] = np.arange(len(seen))
    obs["lm"] = remap[obs["lm"]]
    obs = obs[np.argsort(obs["lm"], kind="stable")]
    return replace(win, obs=obs, lm=np.ascontiguousarray(win.lm[seen]), truth_lm=win.truth_lm[seen])


def _full_lm_tile():
    win = make_window(n_opt_kf=8, n_fixed=2, n_lm=300, obs_per_lm=5, n_cam=1, gp=False, stereo_frac=0.0, seed=61)
    lm = win.obs["lm"]
    first = np.r_[True, lm[1:] != lm[:-1]]
    last = np.r_[lm[1:] != lm[:-1], True]
    return replace(win, obs=win.obs[first | last].copy(), name="full_lm_tile")   # (sorted by landmark, then keyframe)


def _long_sample():
    win = make_window(n_opt_kf=2, n_fixed=1, n_lm=240, obs_per_lm=3, n_cam=1, gp=False, seed=62)
    rows = [(l, 2) for l in range(len(win.lm))] + [(l, l % 2) for l in range(len(win.lm)) if l % 3]
    rows.sort()
    obs = np.zeros(len(rows), win.obs.dtype)
    obs["lm"] = [r[0] for r in rows]
    obs["kf_b"] = [r[1] for r in rows]
    obs["kf_a"] = -1
    obs["kind"] = STEREO
    obs["cam"] = 0
    obs["t"] = win.kfs["time"][obs["kf_b"]]
    obs["w"] = 1.0
    return replace(_remeasure(win, obs, 62), name="long_sample")


def _many_samples():
    win = make_window(n_opt_kf=6, n_lm=200, obs_per_lm=6, n_cam=4, gp=True, seed=63)
    rng = np.random.default_rng(63)
    obs = win.obs.copy()
    gp = wm.is_gp(obs)
    obs["t"][gp] = win.kfs["time"][obs["kf_b"][gp]] - rng.uniform(0.01, 0.08, int(gp.sum()))
    assert len(np.unique(obs["t"][gp])) == gp.sum()
    win = _remeasure(win, obs, 63)
    return replace(wm.stereo_gp(win, frac=0.3, seed=64), name="many_samples")


def _minimal():
    win = make_window(n_opt_kf=2, n_fixed=1, n_lm=20, obs_per_lm=4, n_cam=4, gp=True, seed=65)
    pick = np.nonzero((win.obs["kf_b"] == 2) & (win.obs["kind"] >= MONO))[0][:1]
    obs = win.obs[pick].copy()
    obs["kind"] = STEREO
    win = _remeasure(win, obs, 65)
    assert len(win.obs) == 1 and len(win.lm) == 1
    return replace(win, name="minimal")


CASES = {
    "full_lm_tile": _full_lm_tile,
    "long_sample": _long_sample,
    "many_samples": _many_samples,
    "minimal": _minimal,
    "mixed_rows": lambda: wm.stereo_gp(make_window(n_opt_kf=6, n_lm=300, obs_per_lm=6, n_cam=4, gp=True, seed=66),
                                       frac=0.5, seed=67),
    "heavy": lambda: _spanning(n_opt_kf=20, n_lm=150, n_long=2, seed=68),
    "schur_36": lambda: make_window(n_opt_kf=8, n_fixed=1, n_lm=300, obs_per_lm=6, n_cam=4, gp=True, seed=69),
    "schur_66": lambda: make_window(n_opt_kf=12, n_fixed=1, n_lm=400, obs_per_lm=6, n_cam=4, gp=True, seed=70),
}


@functools.lru_cache(maxsize=None)
def _win(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The oracle's results on the window, computed once and shared by the tests (read-only)."""
    win = _win(name)
    o = orc.Oracle(win)
    chi, res, _ = o.errors()
    H, b, Hll = o.build_system()
    steps = {lam: o.solve(lam) for lam in (1.0, 1e-3)}
    o2 = orc.Oracle(win)
    n, st = o2.optimize(10)
    kf, lm = o2.state()
    return dict(chi=chi, res=res, H=H, b=b, Hll=Hll, steps=steps, n=n, st=st, kf=kf, lm=lm, depth_ok=o2.depth_ok())


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_windows_have_their_tile_shapes():
    """lba_setup_tile_shapes (the host tiling of lba_set_problem, no GPU) on every window."""
    sh = {name: amc_lba.setup_tile_shapes(_win(name)) for name in CASES}
    for name, s in sh.items():
        print(name, s)
        assert s["tiles"] >= 1 and s["obs"] <= TILE_OBS and s["rows"] <= TILE_ROWS
    o = _win("full_lm_tile").obs
    assert (o["kind"] == MONO).all() and (np.bincount(o["lm"]) == 2).all()
    assert sh["full_lm_tile"]["landmarks"] == TILE_LMS and sh["full_lm_tile"]["tiles"] >= 2
    assert (_win("long_sample").obs["kind"] == STEREO).all() and _win("long_sample").kfs["fixed"].sum() == 1
    assert sh["long_sample"]["samples"] <= 3 and sh["long_sample"]["sample_rows"] >= 150
    assert TILE_SMP - 4 <= sh["many_samples"]["samples"] <= TILE_SMP
    assert sh["many_samples"]["samples"] * 9 > 2 * 256   # phase 2: more than two passes of the workgroup
    m = sh["minimal"]
    assert (m["tiles"], m["obs"], m["samples"], m["landmarks"], m["pairs"], m["kfs"], m["schur_entries"]) == \
        (1, 1, 1, 1, 1, 1, 1) and m["rows"] == 3
    k = _win("mixed_rows").obs["kind"]
    assert (k == wm.STEREO_GP).sum() > 100 and (k == wm.MONO_GP).sum() > 100
    assert sh["mixed_rows"]["rows"] > 2 * sh["mixed_rows"]["obs"] - 2 * TILE_OBS + 200   # (3-row groups among them)
    assert sh["heavy"]["seg_tiles"] >= 1 and sh["heavy"]["seg_pairs"] > 16   # (more pose blocks than TILE_KF)
    assert 33 <= sh["schur_36"]["schur_entries"] <= 40 and sh["schur_36"]["kfs"] == 8
    assert 65 <= sh["schur_66"]["schur_entries"] <= 80


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_linearize_and_steps_match_oracle(name):
    win, r = _win(name), _ref(name)
    p = Problem(win)
    res, H, b, Hll = p.linearize()
    dres = np.linalg.norm(res - r["res"]) / np.linalg.norm(r["res"])
    print(f"{name}: residual {dres:.2e}  H {_rel(H, r['H']):.2e}  b {_rel(b, r['b']):.2e}  Hll {_rel(Hll, r['Hll']):.2e}")
    assert dres <= 1e-8, dres
    assert H.shape == r["H"].shape
    assert _rel(H, r["H"]) < 1e-9
    assert _rel(b, r["b"]) < 1e-9
    assert _rel(Hll, r["Hll"]) < 1e-9
    np_ = p.pose_dim
    for lam, (ok_o, dx_o) in r["steps"].items():
        ok, dx = p.solve_step(lam)
        print(f"{name}: lambda {lam:g}: dx poses {_rel(dx[:np_], dx_o[:np_]):.2e}  landmarks {_rel(dx[np_:], dx_o[np_:]):.2e}")
        assert ok == ok_o
        assert _rel(dx[:np_], dx_o[:np_]) <= 1e-6
        assert _rel(dx[np_:], dx_o[np_:]) <= 1e-6
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_optimize_matches_oracle(name):
    win, r = _win(name), _ref(name)
    p = Problem(win)
    n, st = p.optimize(10)
    kf, lm = p.state()
    st_o, kf_o, lm_o = r["st"], r["kf"], r["lm"]
    print(f"{name}: iterations {n} / {r['n']}  trials {st.trials} / {st_o.trials}  chi2 {st.chi2_final:.9e} / "
          f"{st_o.chi2_final:.9e}")
    assert n == r["n"]
    assert st.trials == st_o.trials
    assert st.result == st_o.result
    assert abs(st.chi2_initial - st_o.chi2_initial) <= 1e-9 * st_o.chi2_initial
    assert abs(st.chi2_final - st_o.chi2_final) <= 1e-7 * st_o.chi2_final
    assert _rel(kf["t"], kf_o["t"]) <= 1e-6
    assert _rel(kf["vel"], kf_o["vel"]) <= 1e-5
    q, qo = kf["q"] * np.sign(kf["q"][:, 3:4]), kf_o["q"] * np.sign(kf_o["q"][:, 3:4])
    assert np.abs(q - qo).max() <= 1e-7
    assert _rel(lm, lm_o) <= 1e-6
    _, _, ok = p.eval()
    np.testing.assert_array_equal(ok, r["depth_ok"])
    p.close()


@pytest.mark.gpu
def test_f32_residual_mixed_rows_within_tolerance():
    """The fp32-residual instantiation on the mixed 2- / 3-row window, at tests/test_gpu_f32_residual.py's
    tolerances (and above fp64 rounding: the fp32 kernels ran)."""
    win, r = _win("mixed_rows"), _ref("mixed_rows")
    p = Problem(win, flags=FLAG_F32_RESIDUAL)
    res, H, b, _ = p.linearize()
    dres = np.linalg.norm(res - r["res"]) / np.linalg.norm(r["res"])
    dH, db = _rel(H, r["H"]), _rel(b, r["b"])
    chi, _, _ = p.eval()
    dchi = abs(chi - r["chi"]) / r["chi"]
    ok, dx = p.solve_step(1.0)
    ok_o, dx_o = r["steps"][1.0]
    ddx = _rel(dx, dx_o)
    p.close()
    print(f"mixed_rows f32: residual {dres:.2e}  H {dH:.2e}  b {db:.2e}  chi2 {dchi:.2e}  dx {ddx:.2e}")
    assert 1e-9 < dres <= 1e-3, dres
    assert dH <= 1e-5 and db <= 1e-4, (dH, db)
    assert dchi <= 1e-4, dchi
    assert ok and ok_o
    assert ddx <= 1e-3, ddx
    p = Problem(win, early_stop=0, flags=FLAG_F32_RESIDUAL)
    n, st = p.optimize(10)
    kf, lm = p.state()
    p.close()
    o = orc.Oracle(win, early_stop=0)
    n_o, st_o = o.optimize(10)
    kf_o, lm_o = o.state()
    dchi = abs(st.chi2_final - st_o.chi2_final) / st_o.chi2_final
    dt, dl = _rel(kf["t"], kf_o["t"]), _rel(lm, lm_o)
    print(f"mixed_rows f32: trials {st.trials} / {st_o.trials}  chi2 {dchi:.2e}  kf t {dt:.2e}  lm {dl:.2e}")
    assert n == n_o == 10
    assert dchi <= 1e-3, dchi
    assert dt <= 1e-3 and dl <= 1e-3, (dt, dl)
