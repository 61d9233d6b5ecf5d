"""lba_track (k_track, amc-slam_amd/csrc/lba_track.hip) at its edges against the oracle (orc_track_pose).

tests/test_gpu_track.py compares one batch of regular frames started close to the truth.  The cases of
tests/track_cases.py reach what that batch does not: rejected LM trials (with g2o's stale per-edge chi2 of a
rejected trial state), the stop rules qmax == max_trials, early_stop = 0 and a user lambda, frames with one
sample, without an own-pose sample, with TR_MAXS samples and one more, GP observations stamped at the ends of
the interval, n_obs of 0, 1, 6 | 7 (where the call ends after one round) and 255, 256, 257 (one stride of the
256-thread loops), small frames with the previous frame free, points behind the camera, every observation
an outlier on entry, cur.fixed set on entry, rows in any order, ranges in any order with unused rows between
them.  tests/test_track_cases.py shows on the CPU that each case has its property and is conditioned well
enough for the comparison (integers stable and pose within a tenth of the tolerances under a 1e-9
disturbance of the measurements and under reordered rows, no LM decision taken at the rounding floor of chi2).

Per case one Tracker.track call against orc.track_pose frame by frame: n_good, iterations and every outlier
flag equal, the pose within the tolerances of tests/test_gpu_track.py, and everything that is not an output
byte for byte as it went in.  Then the host side: a batch of more workgroups than the device has CUs gives
every frame bitwise its result alone (the kernel's sums are in fixed order), a Tracker reused over growing and
shrinking batches gives bitwise what a fresh one gives, an empty batch writes nothing, a 17-sample frame is
refused with LBA_E_LIMIT before any launch.  The parity test prints the margins it measures (pytest -s).
"""
import functools

import numpy as np
import pytest

import track_cases as tc
from amc_lba import LbaError
from amc_lba.abi import LBA_E_LIMIT
from amc_lba.track import Tracker, track_config

pytestmark = pytest.mark.gpu

NAMES = list(tc.CASES)
N_BATCH = 300      # frames of the tiled batch: more workgroups than an MI355X has CUs (256)


def _assert_untouched(frames, obs, cams, fr_g, ob_g, cams_g):
    """Everything lba_track does not return is byte for byte what went in."""
    assert fr_g["prev"].tobytes() == frames["prev"].tobytes()
    for f in ("time", "bf", "fixed", "pad"):
        assert fr_g["cur"][f].tobytes() == frames["cur"][f].tobytes(), f
    for f in ("obs0", "n_obs"):
        assert fr_g[f].tobytes() == frames[f].tobytes(), f
    for f in obs.dtype.names:
        if f != "outlier":
            assert ob_g[f].tobytes() == obs[f].tobytes(), f
    unused = ~tc.used_rows(frames, len(obs))
    np.testing.assert_array_equal(ob_g["outlier"][unused], obs["outlier"][unused])
    assert cams_g.tobytes() == cams.tobytes()


def _assert_bitwise(fr_a, ob_a, fr_b, ob_b, what):
    assert fr_a.tobytes() == fr_b.tobytes(), what
    assert ob_a.tobytes() == ob_b.tobytes(), what


@pytest.mark.parametrize("name", NAMES)
def test_case_matches_oracle(name):
    cfg, frames, obs, cams = tc.case(name)
    fr_o, ob_o = tc.reference(name)
    cams_g = cams.copy()
    fr_g, ob_g = Tracker(cfg).track(frames.copy(), obs.copy(), cams_g)
    worst = np.zeros(3)
    for f in range(len(frames)):
        g, o = fr_g[f], fr_o[f]
        s = tc.frame_slice(frames[f])
        d = tc.pose_diff(g["cur"], o["cur"])
        worst = np.maximum(worst, d)
        print(f"{name}[{f}]: n_obs {o['n_obs']} n_good {g['n_good']} / {o['n_good']}  iterations {g['iterations']} / "
              f"{o['iterations']}  flags differing {int((ob_g['outlier'][s] != ob_o['outlier'][s]).sum())}  "
              f"t {d[0]:.2e}  q {d[1]:.2e}  vel {d[2]:.2e}")
    print(f"{name}: GPU vs oracle  t {worst[0]:.2e}  q {worst[1]:.2e}  vel {worst[2]:.2e}")
    for f in range(len(frames)):
        g, o = fr_g[f], fr_o[f]
        s = tc.frame_slice(frames[f])
        assert g["n_good"] == o["n_good"] and g["iterations"] == o["iterations"], f
        np.testing.assert_array_equal(ob_g["outlier"][s], ob_o["outlier"][s], err_msg=f"frame {f}")
        dt, dq, dv = tc.pose_diff(g["cur"], o["cur"])
        assert dt <= tc.TOL_T and dq <= tc.TOL_Q and dv <= tc.TOL_V, (f, dt, dq, dv)
    _assert_untouched(frames, obs, cams, fr_g, ob_g, cams_g)


# ------------------------------------------------------------------ the host side: batches, reuse, refusals
@functools.lru_cache(maxsize=None)
def _sources():
    """Every frame of every case that runs under the default configuration (all but `controller`), with its
    observations and its case's cameras: 0 to 1265 observations, 1 to 16 cameras, 0 to 16 samples."""
    out = []
    for name in NAMES:
        if name.startswith("controller_"):
            continue
        _, frames, obs, cams = tc.case(name)
        for f in range(len(frames)):
            out.append((frames[f:f + 1], obs[tc.frame_slice(frames[f])], cams))
    return out


@functools.lru_cache(maxsize=None)
def _batch():
    """N_BATCH frames tiled from _sources(), their observations back to back, the cases' camera tables
    concatenated (each frame's observations point into its own case's part).  Returns (frames, obs, cams,
    source index per frame), read-only."""
    src = _sources()
    cam_parts, cam0, at = [], {}, 0
    for _, _, cams in src:
        if id(cams) not in cam0:
            cam0[id(cams)] = at
            cam_parts.append(cams)
            at += len(cams)
    frames, obs, which, n = [], [], [], 0
    for i in range(N_BATCH):
        j = i % len(src)
        F, o, cams = src[j]
        F, o = F.copy(), o.copy()
        F["obs0"] = n
        o["cam"] += cam0[id(cams)]
        n += len(o)
        frames.append(F)
        obs.append(o)
        which.append(j)
    out = (np.concatenate(frames), np.concatenate(obs), np.concatenate(cam_parts))
    for a in out:
        a.setflags(write=False)
    return out + (which,)


@functools.lru_cache(maxsize=None)
def _batch_result():
    """The batch on a fresh Tracker, once."""
    frames, obs, cams, _ = _batch()
    fr, ob = Tracker(track_config()).track(frames.copy(), obs.copy(), cams.copy())
    fr.setflags(write=False)
    ob.setflags(write=False)
    return fr, ob


def test_batch_frames_are_independent():
    frames, obs, cams, which = _batch()
    assert len(frames) == N_BATCH > 256 and len(_sources()) >= 40
    assert len(set(int(n) for n in frames["n_obs"])) >= 10          # mixed sizes
    fr_b, ob_b = _batch_result()
    alone = []
    for F, o, c in _sources():
        a = F.copy()
        a["obs0"] = 0
        alone.append(Tracker(track_config()).track(a, o.copy(), c.copy()))
    for i in range(N_BATCH):
        fr_a, ob_a = alone[which[i]]
        g = fr_b[i]
        for f in ("q", "t", "vel"):
            assert g["cur"][f].tobytes() == fr_a[0]["cur"][f].tobytes(), (i, f)
        assert g["n_good"] == fr_a[0]["n_good"] and g["iterations"] == fr_a[0]["iterations"], i
        np.testing.assert_array_equal(ob_b["outlier"][tc.frame_slice(frames[i])], ob_a["outlier"], err_msg=f"frame {i}")
    _assert_untouched(frames, obs, cams, fr_b, ob_b, cams)


def test_tracker_reuse_over_growing_and_shrinking_batches():
    frames, obs, cams, _ = _batch()
    fr_b, ob_b = _batch_result()
    cfg = track_config()
    F1, o1, c1 = _sources()[2]
    F0 = F1.copy()
    F0["n_obs"] = 0
    t = Tracker(cfg)
    calls = [("batch", frames, obs, cams), ("one frame", F1, o1, c1), ("no observation", F0, o1[:0], c1),
             ("batch again", frames, obs, cams)]
    for what, fr, ob, cm in calls:
        got = t.track(fr.copy(), ob.copy(), cm.copy())
        if fr is frames:
            want = (fr_b, ob_b)
        else:
            want = Tracker(cfg).track(fr.copy(), ob.copy(), cm.copy())
        _assert_bitwise(got[0], got[1], want[0], want[1], what)


def test_empty_batch_writes_nothing():
    _, frames, obs, cams = tc.case("regular_c4-fix")
    fr, ob = Tracker(track_config()).track(frames[:0].copy(), obs.copy(), cams.copy())
    assert len(fr) == 0 and ob.tobytes() == obs.tobytes()
    fr, ob = Tracker(track_config()).track(frames[:0].copy(), obs[:0].copy(), cams.copy())
    assert len(fr) == 0 and len(ob) == 0


@pytest.mark.parametrize("fix", (True, False))
def test_seventeen_samples_are_refused(fix):
    cfg, frames, obs, cams = tc.case_samples(fix, 17)
    f, o = frames.copy(), obs.copy()
    with pytest.raises(LbaError) as e:
        Tracker(cfg).track(f, o, cams)
    assert e.value.code == LBA_E_LIMIT
    assert f.tobytes() == frames.tobytes() and o.tobytes() == obs.tobytes()


@pytest.mark.parametrize("fix", (True, False))
def test_shuffled_rows_give_the_permuted_flags(fix):
    """The host's permutation by sample and its scatter of the flags back, on the device's own results: the
    rows in another order give the same flags row for row, and the pose within the tolerances (another
    summation order, so not bitwise)."""
    cfg, frames, obs, cams = tc.case(f"shuffled_obs-{tc.tag(fix)}")
    _, _, obs_u, _ = tc.case_shuffled_obs(fix, shuffle=False)
    perm = tc.shuffle_perm(len(obs))
    t = Tracker(cfg)
    fr_s, ob_s = t.track(frames.copy(), obs.copy(), cams.copy())
    fr_u, ob_u = t.track(frames.copy(), obs_u.copy(), cams.copy())
    np.testing.assert_array_equal(ob_s["outlier"], ob_u["outlier"][perm])
    assert fr_s[0]["n_good"] == fr_u[0]["n_good"] and fr_s[0]["iterations"] == fr_u[0]["iterations"]
    dt, dq, dv = tc.pose_diff(fr_s[0]["cur"], fr_u[0]["cur"])
    print(f"shuffled vs unshuffled on the GPU: t {dt:.2e}  q {dq:.2e}  vel {dv:.2e}")
    assert dt <= tc.TOL_T and dq <= tc.TOL_Q and dv <= tc.TOL_V
