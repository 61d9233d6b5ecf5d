"""k_lin_schur's packed inputs at the shapes where their staging can go wrong.

The sweep reads one descriptor per tile workgroup (dispatch order) and one 64-byte record per observation, and stages
a regular tile's sample poses (by tile-local sample, ob_row >> 16), landmarks (by lm - lm0), the keyframes' bf and,
with at most 8 cameras, the cameras' projection records in LDS before phase 1 (lba_device.hpp TileDesc / ObsRec,
lba_kernels.hip).  Each window below reaches one limit or one other path of that staging; each is compared with the
CPU oracle at tests/test_gpu_parity.py's tolerances: lba_linearize (residuals, H_pp, b, H_ll), one solve_step at
lambda = 1, and optimize(10) in the queued and the host loop.

  smp_64         GP observations each at its own time stamp, four per landmark: a tile of exactly TILE_SMP = 64 samples
  lm_obs_full    two mono observations per landmark: tiles of TILE_LMS = 64 landmarks and TILE_OBS = 128 observations
  one_obs        one stereo observation of one landmark
  stereo_gp      LBA_STEREO_GP among LBA_MONO_GP observations (3-row and 2-row observations in one tile)
  cams_20        20 cameras: more than the 8 staged in LDS, every lane loads its own camera record
  cams_8         exactly 8 cameras: the last size that is staged
  free_ext       free extrinsics: the camera records differ between the two state buffers
  heavy          landmarks seen from more keyframes than a tile holds: segment tiles (per-lane gathers, no staging)
  fixed_scattered / fixed_only_landmarks   fixed keyframes anywhere, landmarks without a free pose vertex
  (stereo_gp again with LBA_FLAG_F32_RESIDUAL, at tests/test_gpu_f32_residual.py's tolerances)

Bitwise cases: lba_set_state with changed keyframe records (bf included) against a fresh lba_set_problem of that state
(bf is read from the live keyframe record, never from a set-up copy), engine reuse across windows of different shape
against fresh engines (stale descriptors), and a repeated run.

The CPU test asserts with lba_setup_tile_shapes (the host tiling, no device) that every window has its shape.
"""
import functools
from dataclasses import replace

import numpy as np
import pytest

import amc_lba
import orc
import window_mutations as wm
from amc_lba import Problem
from amc_lba.abi import FLAG_F32_RESIDUAL, FLAG_HOST_LOOP, MONO_GP, STEREO
from amc_lba.synth import make_window, with_free_extrinsics
from test_gpu_sweep_lanes import _full_lm_tile, _minimal, _remeasure
from test_heavy_landmarks import _spanning

TILE_LMS, TILE_SMP, TILE_ROWS, TILE_OBS, ST_CAMS = 64, 64, 288, 128, 8


def _smp_64():
    """Every landmark keeps exactly four LBA_MONO_GP observations, each at a time stamp of its own: a tile's samples
    are its observations, so the greedy cut closes the first tiles at 16 landmarks = 64 samples."""
    win = make_window(n_opt_kf=6, n_lm=200, obs_per_lm=8, n_cam=4, gp=True, stereo_frac=0.0, seed=81)
    rng = np.random.default_rng(81)
    obs = win.obs[win.obs["kind"] == MONO_GP].copy()
    obs["t"] = win.kfs["time"][obs["kf_b"]] - rng.uniform(0.01, 0.08, len(obs))
    assert len(np.unique(obs["t"])) == len(obs)
    win = _remeasure(win, obs, 81)
    o = win.obs
    rank = np.arange(len(o)) - np.searchsorted(o["lm"], o["lm"])   # (sorted by landmark) index within the landmark
    full = np.bincount(o["lm"], minlength=len(win.lm)) >= 4
    keep = full[o["lm"]] & (rank < 4)
    obs = o[keep].copy()
    seen = np.unique(obs["lm"])
    remap = -np.ones(len(win.lm), np.int64)
    remap[seen] = np.arange(len(seen))
    obs["lm"] = remap[obs["lm"]]
    return replace(win, obs=obs, lm=np.ascontiguousarray(win.lm[seen]), truth_lm=win.truth_lm[seen], name="smp_64")


SMALL = dict(n_opt_kf=6, n_lm=300, obs_per_lm=6, gp=True)
CASES = {
    "smp_64": _smp_64,
    "lm_obs_full": _full_lm_tile,
    "one_obs": _minimal,
    "stereo_gp": lambda: wm.stereo_gp(make_window(n_cam=4, seed=82, **SMALL), frac=0.5, seed=83),
    "cams_20": wm.many_cams,
    "cams_8": lambda: make_window(n_cam=ST_CAMS, seed=84, **SMALL),
    "free_ext": lambda: with_free_extrinsics(make_window(n_cam=4, seed=85, **SMALL)),
    "heavy": lambda: _spanning(n_opt_kf=20, n_lm=150, n_long=2, seed=86),
    "fixed_scattered": wm.CASES["fixed_scattered"],
    "fixed_only_landmarks": wm.CASES["fixed_only_landmarks"],
}
LOOPS = {"queued": 0, "host_loop": FLAG_HOST_LOOP}


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
    step = o.solve(1.0)
    o2 = orc.Oracle(win)
    n, st = o2.optimize(10)
    kf, lm = o2.state()
    return dict(chi=chi, res=res, H=H, b=b, Hll=Hll, step=step, n=n, st=st, kf=kf, lm=lm, depth_ok=o2.depth_ok())


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_windows_have_their_tile_shapes():
    """lba_setup_tile_shapes (the host tiling of lba_set_problem, no GPU) on every window."""
    sh = {name: amc_lba.setup_tile_shapes(_win(name)) for name in CASES}
    for name, s in sh.items():
        print(name, s)
        assert s["tiles"] >= 1 and s["obs"] <= TILE_OBS and s["rows"] <= TILE_ROWS and s["samples"] <= TILE_SMP
    o = _win("smp_64").obs
    assert (o["kind"] == MONO_GP).all() and (np.bincount(o["lm"]) == 4).all() and len(np.unique(o["t"])) == len(o)
    assert sh["smp_64"]["samples"] == TILE_SMP and sh["smp_64"]["tiles"] >= 2
    assert sh["lm_obs_full"]["landmarks"] == TILE_LMS and sh["lm_obs_full"]["obs"] == TILE_OBS
    assert sh["lm_obs_full"]["tiles"] >= 2
    m = sh["one_obs"]
    assert (m["tiles"], m["obs"], m["samples"], m["landmarks"]) == (1, 1, 1, 1) and len(_win("one_obs").obs) == 1
    k = _win("stereo_gp").obs["kind"]
    assert (k == wm.STEREO_GP).sum() > 100 and (k == MONO_GP).sum() > 100
    assert len(_win("cams_20").cams) > ST_CAMS and len(np.unique(_win("cams_20").obs["cam"])) > ST_CAMS
    assert len(_win("cams_8").cams) == ST_CAMS and len(np.unique(_win("cams_8").obs["cam"])) == ST_CAMS
    assert (_win("free_ext").cams["ext_free"] != 0).any()
    assert sh["heavy"]["seg_tiles"] >= 1 and sh["heavy"]["seg_obs"] >= 1
    f = _win("fixed_scattered").kfs["fixed"]
    assert f[4] and f[10] and not f[3]
    w = _win("fixed_only_landmarks")
    on_fixed = w.kfs["fixed"][w.obs["kf_b"]] != 0
    assert all(on_fixed[w.obs["lm"] == l].all() and (w.obs["lm"] == l).sum() == 2 for l in range(12))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_linearize_and_step_match_oracle(name):
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
    ok_o, dx_o = r["step"]
    ok, dx = p.solve_step(1.0)
    print(f"{name}: dx poses {_rel(dx[:np_], dx_o[:np_]):.2e}  landmarks {_rel(dx[np_:], dx_o[np_:]):.2e}")
    assert ok == ok_o
    assert _rel(dx[:np_], dx_o[:np_]) <= 1e-6
    assert _rel(dx[np_:], dx_o[np_:]) <= 1e-6
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("name", list(CASES))
def test_optimize_matches_oracle(name, loop):
    win, r = _win(name), _ref(name)
    p = Problem(win, flags=LOOPS[loop])
    n, st = p.optimize(10)
    kf, lm = p.state()
    st_o, kf_o, lm_o = r["st"], r["kf"], r["lm"]
    print(f"{name}[{loop}]: iterations {n} / {r['n']}  trials {st.trials} / {st_o.trials}  chi2 {st.chi2_final:.9e} / "
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
def test_f32_residual_within_tolerance():
    """The <true> instantiation on the mixed 2- / 3-row window, at tests/test_gpu_f32_residual.py's tolerances (and
    above fp64 rounding: the fp32 kernels ran)."""
    win, r = _win("stereo_gp"), _ref("stereo_gp")
    p = Problem(win, flags=FLAG_F32_RESIDUAL)
    res, H, b, _ = p.linearize()
    dres = np.linalg.norm(res - r["res"]) / np.linalg.norm(r["res"])
    dH, db = _rel(H, r["H"]), _rel(b, r["b"])
    ok, dx = p.solve_step(1.0)
    ok_o, dx_o = r["step"]
    ddx = _rel(dx, dx_o)
    p.close()
    print(f"stereo_gp f32: residual {dres:.2e}  H {dH:.2e}  b {db:.2e}  dx {ddx:.2e}")
    assert 1e-9 < dres <= 1e-3, dres
    assert dH <= 1e-5 and db <= 1e-4, (dH, db)
    assert ok and ok_o
    assert ddx <= 1e-3, ddx
    for loop, flags in LOOPS.items():
        p = Problem(win, early_stop=0, flags=FLAG_F32_RESIDUAL | flags)
        n, st = p.optimize(10)
        kf, lm = p.state()
        p.close()
        o = orc.Oracle(win, early_stop=0)
        n_o, st_o = o.optimize(10)
        kf_o, lm_o = o.state()
        dchi = abs(st.chi2_final - st_o.chi2_final) / st_o.chi2_final
        dt, dl = _rel(kf["t"], kf_o["t"]), _rel(lm, lm_o)
        print(f"stereo_gp f32 [{loop}]: trials {st.trials} / {st_o.trials}  chi2 {dchi:.2e}  kf t {dt:.2e}  lm {dl:.2e}")
        assert n == n_o == 10
        assert dchi <= 1e-3, dchi
        assert dt <= 1e-3 and dl <= 1e-3, (dt, dl)


def _lin_bytes(p):
    """What the bitwise cases compare: lba_linearize's residuals, b and H_ll and the step of lba_solve_step, which
    sums the same H_pp partials into the reduced system.  lba_linearize's dense H_pp itself is left out: both lanes
    (i, j) and (j, i) of a diagonal block write both mirrored elements of it, from partial sums that are not bitwise
    symmetric (assemble_item), so its last bit there depends on which store lands last, on any build."""
    res, _, b, Hll = p.linearize()
    ok, dx = p.solve_step(1.0)
    return res.tobytes(), b.tobytes(), Hll.tobytes(), bool(ok), dx.tobytes()


@pytest.mark.gpu
def test_set_state_with_changed_bf_is_bitwise_a_fresh_problem():
    """lba_set_state with other keyframe records (pose, velocity and the stereo bf) and landmarks, then linearise and
    step: bit for bit a fresh lba_set_problem of that state.  The window has stereo observations, so bf enters."""
    win = wm.stereo_gp(make_window(n_cam=4, seed=87, stereo_frac=0.9, **SMALL), frac=0.5, seed=88)
    assert (win.obs["kind"] == STEREO).sum() > 20 and (win.obs["kind"] == wm.STEREO_GP).sum() > 50
    rng = np.random.default_rng(89)
    kfs = win.kfs.copy()
    kfs["bf"] = kfs["bf"] * (1.0 + 0.05 * rng.random(len(kfs)))
    kfs["t"] += rng.normal(0, 1e-3, kfs["t"].shape)
    kfs["vel"] += rng.normal(0, 1e-3, kfs["vel"].shape)
    lm = win.lm + rng.normal(0, 1e-3, win.lm.shape)
    p = Problem(win)
    before = _lin_bytes(p)
    p.set_state(kfs, lm)
    moved = _lin_bytes(p)
    p.close()
    p = Problem(replace(win, kfs=kfs, lm=lm))
    fresh = _lin_bytes(p)
    p.close()
    assert moved[0] != before[0]
    assert moved == fresh
    # bf alone
    kfs2 = win.kfs.copy()
    kfs2["bf"] = kfs["bf"]
    p = Problem(win)
    p.set_state(kfs2, None)
    moved = _lin_bytes(p)
    p.close()
    p = Problem(replace(win, kfs=kfs2))
    fresh = _lin_bytes(p)
    p.close()
    assert moved[0] != before[0]
    assert moved == fresh


def _run(p):
    n, st = p.optimize(6)
    kf, lm = p.state()
    return n, st.trials, st.chi2_final, st.lambda_final, kf.tobytes(), lm.tobytes()


@pytest.mark.gpu
def test_engine_reuse_across_shapes_is_bitwise_fresh():
    """One engine through windows of different tile counts and shapes (stale descriptors or records would show):
    every run is bit for bit a fresh engine's."""
    names = ["smp_64", "one_obs", "cams_20", "lm_obs_full", "heavy", "smp_64"]
    p = Problem(_win(names[0]), early_stop=0)
    for i, name in enumerate(names):
        if i:
            p.set_window(replace(_win(name), cfg=dict(_win(name).cfg, early_stop=0)))
        got = _lin_bytes(p) + _run(p)
        f = Problem(_win(name), early_stop=0)
        want = _lin_bytes(f) + _run(f)
        f.close()
        assert got == want, name
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["smp_64", "free_ext"])
def test_repeated_run_is_bit_identical(name):
    runs = []
    for _ in range(2):
        p = Problem(_win(name), early_stop=0)
        runs.append(_lin_bytes(p) + _run(p))
        p.close()
    assert runs[0] == runs[1]
