"""Named inputs of lba_sim3_ransac, shared by the CPU tests (tests/test_sim3_ransac_cases.py) and the GPU tests
(tests/test_gpu_sim3_ransac.py), with the fp64 and float32 restatements (tests/sim3_ransac_oracle.py) of each,
computed once.  Sizes are the smallest at which a lane map (64 rows per ballot, 64 hypotheses per selection chunk) or
the selection can go wrong.

A case is (pairs, corr, samples, cams, n_cam) plus `check`, its property on the fp64 restatement.

M_GATE, the margin inside which an inlier flag counts as unsettled, is at least 4 x the largest gate margin at which a
float32 and an fp64 comparison of one error with its gate disagree over all cases (measured by
scripts/sim3_ransac_margins.py into profiles/sim3_ransac_margins.log; tests/test_sim3_ransac_cases.py asserts that it
covers the measurement).
"""
import functools

import numpy as np

import sim3_ransac_oracle as ro
from amc_lba.sim3_ransac import S3R_CORR_DTYPE, S3R_PAIR_DTYPE, make_sim3_ransac_pairs

# profiles/sim3_ransac_margins.log: NO float32 / fp64 disagreement among the 295 563 flags of the cases and six further
# seeds (6 of them lie within 1e-3 of a gate), so 4 x the measurement is 0 and the margin falls back on the formats:
# float32's 6e-8 on image coordinates of up to 1000 px through the ~8 operations of the transfer is 5e-4 px, on a
# difference of 3 px at the level-0 gate of 9 px^2 that is 2 x 5e-4 / 3 = 3e-4 relative, rounded up.
M_GATE = 1e-3
GAP_MIN = 1e-6        # a transform is settled when its relative eigen-gap is at least this
S12_F32_BOUND = 2e-3  # float32 vs fp64 S12 of settled transforms, relative to max(1, |.|): float eps (6e-8) x the
                      # conditioning of a three-point fit (baselines of decimetres at ranges of tens of metres, ~1e4)


class Case:
    def __init__(self, pairs, corr, samples, cams, n_cam=4, check=None):
        self.pairs, self.corr, self.samples, self.cams, self.n_cam, self.check = pairs, corr, samples, cams, n_cam, check

    def pair_inputs(self, p):
        P = self.pairs[p]
        return (P, self.corr[P["corr0"]:P["corr0"] + P["n_corr"]], self.samples[P["hyp0"]:P["hyp0"] + P["n_hyp"]],
                self.cams[P["cam0"]:P["cam0"] + 2 * self.n_cam])

    def oracle(self, dtype=np.float64):
        return [ro.run(*self.pair_inputs(p), self.n_cam, dtype) for p in range(len(self.pairs))]


def _gen(**kw):
    kw.setdefault("n_corr", 40)
    kw.setdefault("n_hyp", 65)
    kw.setdefault("min_inliers", 15)
    return Case(*make_sim3_ransac_pairs(**kw)[:4], n_cam=kw.get("n_cam", 4))


def _counts(c, p=0):
    return ro.run(*c.pair_inputs(p), c.n_cam)


def _is(**want):
    def check(res):
        for k, v in want.items():
            assert res[0][k] == v, (k, res[0][k], v)
    return check


def _sized(n_corr, n_hyp, seed):
    mi = 2 if n_corr == 3 else min(15, n_corr // 3)
    c = _gen(n_corr=n_corr, n_hyp=n_hyp, seed=seed, min_inliers=mi, outlier_frac=0.0 if n_corr == 3 else 0.3)
    if n_corr > 64 and n_hyp:
        # the last row (the second ballot word's last lane in use) is an inlier of the best hypothesis: swap it in
        r = _counts(c)
        a, b = n_corr - 1, int(np.flatnonzero(r["inlier"][r["count"].argmax()])[0])
        c.corr[[a, b]] = c.corr[[b, a]]
        sa, sb = c.samples == a, c.samples == b
        c.samples[sa], c.samples[sb] = b, a

    def check(res):
        assert res[0]["inlier"].shape == (n_hyp, n_corr)
        if n_hyp == 0:
            assert res[0]["best_hyp"] == -1 and res[0]["converged"] == 0 and not res[0]["row_inlier"].any()
        elif n_corr > 3 and n_hyp >= 63:
            assert res[0]["count"].max() > n_corr // 2       # the generator's inliers are found
            if n_corr > 64:
                assert res[0]["inlier"][res[0]["count"].argmax(), 64:].any()   # beyond the first ballot word
    c.check = check
    return c


def _n_corr_equals_min_inliers():
    c = _gen(n_corr=15, n_hyp=1, seed=31, min_inliers=15, outlier_frac=0.0)
    c.check = _is(best_hyp=0, converged=0)      # at most 15 inliers, and 15 > 15 does not hold
    return c


def _count_equals_min_inliers():
    c = _gen(seed=32)
    c.pairs["min_inliers"] = _counts(c)["count"].max()

    def check(res):
        r = res[0]
        assert r["converged"] == 0 and r["n_inliers"] == c.pairs["min_inliers"][0]
        assert r["best_hyp"] == np.flatnonzero(r["count"] == r["count"].max())[-1]
    c.check = check
    return c


def _reordered(seed, order, min_of):
    """the triples reordered by their fp64 count (`order` maps the count array to a permutation), min_inliers from it"""
    c = _gen(seed=seed)
    cnt = _counts(c)["count"]
    perm = order(cnt)
    c.samples[:] = c.samples[perm]
    c.pairs["min_inliers"] = min_of(cnt[perm])
    return c


def _converge_first():
    c = _reordered(33, lambda n: np.argsort(-n, kind="stable"), lambda n: n[0] - 1)
    c.check = _is(best_hyp=0, converged=1)
    return c


def _converge_last():
    # only the last hypothesis exceeds min_inliers: every other triple that does is replaced by the worst one
    c = _gen(seed=34)
    cnt = _counts(c)["count"]
    top, low = int(cnt.argmax()), int(cnt.argmin())
    c.pairs["min_inliers"] = mi = int(cnt[top]) - 1
    keep = c.samples[top].copy()
    c.samples[cnt > mi] = c.samples[low]
    c.samples[-1] = keep

    def check(res):
        n = res[0]["count"]
        assert (n[:-1] <= mi).all() and n[-1] > mi and res[0]["best_hyp"] == len(n) - 1 and res[0]["converged"] == 1
    c.check = check
    return c


def _converge_ignores_better():
    c = _reordered(35, lambda n: np.argsort(n, kind="stable"), lambda n: n[len(n) // 2] - 1)

    def check(res):
        r = res[0]
        assert r["converged"] == 1 and r["count"].max() > r["n_inliers"] and r["best_hyp"] < r["count"].argmax()
        assert (r["count"][:r["best_hyp"]] <= c.pairs["min_inliers"][0]).all()
    c.check = check
    return c


def _tie_later_wins():
    c = _gen(seed=36)
    cnt = _counts(c)["count"]
    top = int(cnt.argmax())
    c.samples[-3] = c.samples[top]            # the same triple again: the same count, later
    c.pairs["min_inliers"] = cnt.max()

    def check(res):
        r = res[0]
        ties = np.flatnonzero(r["count"] == r["count"].max())
        assert len(ties) >= 2 and r["converged"] == 0 and r["best_hyp"] == ties[-1]
    c.check = check
    return c


def _all_outliers():
    c = _gen(seed=37)
    c.corr["max_err1"] = 0.0                  # err < 0 never holds: every count is 0, and 0 >= 0 keeps the last

    def check(res):
        r = res[0]
        assert not r["count"].any() and r["converged"] == 0 and r["n_inliers"] == 0
        assert r["best_hyp"] == np.flatnonzero(~r["degenerate"])[-1]
    c.check = check
    return c


def _identity_rotation():
    c = _gen(seed=38)
    c.corr["X2b"] = c.corr["X1b"]             # M symmetric, q = (1, 0, 0, 0): every hypothesis is degenerate

    def check(res):
        assert res[0]["degenerate"].all()
        _is(best_hyp=-1, converged=0, n_inliers=0)(res)
    c.check = check
    return c


def _degenerate_first():
    c = _gen(seed=39, n_corr=60)
    a = c.samples[0]
    c.corr["X2b"][a] = c.corr["X1b"][a]

    def check(res):
        r = res[0]
        assert r["degenerate"][0] and not r["degenerate"][1:].all() and r["best_hyp"] > 0 and r["converged"] == 1
    c.check = check
    return c


def _scale(fix_scale):
    c = _gen(seed=40 + fix_scale, s_true=1.05, fix_scale=bool(fix_scale), n_hyp=64)

    def check(res):
        r = res[0]
        if fix_scale:
            assert (r["s"] == 1).all() and r["converged"] == 0     # a 5 % scale error leaves too few inliers
        else:
            assert r["converged"] == 1 and abs(r["s"][r["best_hyp"]] - 1.05) < 0.02
    c.check = check
    return c


def _camera_combinations():
    c = _gen(seed=42, n_corr=48, n_cam=4, cam_yaws=(-0.45, -0.15, 0.15, 0.45), pairing="spread")

    def check(res):
        seen = {(int(a), int(b)) for a, b in zip(c.corr["cam1"], c.corr["cam2"])}
        assert len(seen) == 16 and res[0]["converged"] == 1
    c.check = check
    return c


def _mixed_octaves():
    c = _gen(seed=43, n_octaves=4)

    def check(res):
        assert set(c.corr["max_err1"]) == set(c.corr["max_err2"]) == {9.0, 13.0, 19.0, 27.0}   # floor(9.210 * 1.2^(2k))
        assert res[0]["converged"] == 1
    c.check = check
    return c


def _behind_and_z0():
    c = _gen(seed=44)
    P = c.pairs[0]
    # row 0: in front of nothing: the body origin seen by a camera whose tcb has z = 0 exactly, so Xc.z = 0
    c.cams["t"][P["cam0"] + c.corr["cam1"][0], 2] = 0.0
    c.corr["X1b"][0] = 0.0
    # row 1: both body points mirrored through the body origin: behind their cameras, no depth test
    c.corr["X1b"][1] *= -1
    c.corr["X2b"][1] *= -1

    def check(res):
        r = res[0]
        assert not r["inlier"][:, 0].any() and not np.isfinite(r["err1"][:, 0]).any()
        assert np.isfinite(r["err1"][~r["nonfinite"], 1]).all() and r["converged"] == 1
    c.check = check
    return c


def _coincident_and_nan():
    c = _gen(seed=45, n_corr=41)
    a = c.samples[0]
    c.corr["X1b"][a] = c.corr["X1b"][a[0]]    # an exactly coincident triple: N = 0, degenerate by the solver's convention
    c.corr["X2b"][a] = c.corr["X2b"][a[0]]
    c.corr["X2b"][40] = np.nan                # quirk (c): a transform that is not finite scores 0
    c.samples[c.samples == 40] = 39 if 39 not in a else 38
    c.samples[1] = (40, *[r for r in range(41) if r not in a][:2])

    def check(res):
        r = res[0]
        assert r["degenerate"][0] and r["nonfinite"][1] and not r["degenerate"][1] and r["count"][1] == 0
        assert not r["inlier"][:, 40].any()
    c.check = check
    return c


def _nan_selected():
    c = _all_outliers()
    c.corr["X2b"][5] = np.nan
    c.samples[-1] = (5, 6, 7)

    def check(res):
        r = res[0]
        assert r["best_hyp"] == len(r["count"]) - 1 and r["nonfinite"][-1] and r["n_inliers"] == 0    # through 0 >= 0
    c.check = check
    return c


def _shuffled():
    base = _gen(seed=46)
    perm = np.random.default_rng(46).permutation(len(base.corr))
    inv = np.argsort(perm)
    c = Case(base.pairs.copy(), base.corr[perm].copy(), inv[base.samples].astype(np.int32), base.cams.copy())
    want = _counts(base)

    def check(res):
        assert (res[0]["count"] == want["count"]).all() and res[0]["best_hyp"] == want["best_hyp"]
        assert (res[0]["row_inlier"] == want["row_inlier"][perm]).all()
    c.check = check
    return c


def _ranges_out_of_order():
    a, b = _gen(seed=47, n_corr=30, n_hyp=20), _gen(seed=48, n_corr=70, n_hyp=66)
    pairs = np.concatenate([a.pairs, b.pairs])
    # pair 0's rows, triples and cameras lie behind pair 1's, with unused rows in between
    pad = np.zeros(3, S3R_CORR_DTYPE)
    corr = np.concatenate([b.corr, pad, a.corr])
    samples = np.concatenate([np.zeros((2, 3), np.int32), b.samples, a.samples])
    cams = np.concatenate([b.cams, a.cams])
    pairs["corr0"] = (len(b.corr) + 3, 0)
    pairs["hyp0"] = (2 + len(b.samples), 2)
    pairs["cam0"] = (len(b.cams), 0)
    c = Case(pairs, corr, samples, cams)
    wa, wb = _counts(a), _counts(b)

    def check(res):
        assert (res[0]["count"] == wa["count"]).all() and (res[1]["count"] == wb["count"]).all()
    c.check = check
    return c


BUILDERS = {
    **{f"n_corr_{n}": functools.partial(_sized, n, 6 if n == 3 else 65, 100 + n) for n in (3, 63, 64, 65, 128, 129)},
    **{f"n_hyp_{h}": functools.partial(_sized, 100 if h == 300 else 40, h, 200 + h) for h in (0, 1, 63, 64, 65, 300)},
    "n_corr_equals_min_inliers": _n_corr_equals_min_inliers,
    "count_equals_min_inliers": _count_equals_min_inliers,
    "converge_first": _converge_first,
    "converge_last": _converge_last,
    "converge_ignores_better": _converge_ignores_better,
    "tie_later_wins": _tie_later_wins,
    "all_outliers": _all_outliers,
    "identity_rotation": _identity_rotation,
    "degenerate_first": _degenerate_first,
    "free_scale": functools.partial(_scale, 0),
    "fix_scale": functools.partial(_scale, 1),
    "camera_combinations": _camera_combinations,
    "mixed_octaves": _mixed_octaves,
    "behind_and_z0": _behind_and_z0,
    "coincident_and_nan": _coincident_and_nan,
    "nan_selected": _nan_selected,
    "shuffled": _shuffled,
    "ranges_out_of_order": _ranges_out_of_order,
}
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(Case, fp64 restatement per pair, float32 restatement per pair); computed once, not to be modified"""
    c = BUILDERS[name]()
    return c, c.oracle(np.float64), c.oracle(np.float32)


def run_device(tracker, c):
    """lba_sim3_ransac on copies of the case's arrays: (pairs, corr, hyp)"""
    return tracker.sim3_ransac(c.pairs.copy(), c.corr.copy(), c.samples.copy(), c.cams.copy(), c.n_cam)


def device_gaps(c, r64, got):
    """The device's outputs against the fp64 restatement, pair by pair.  Returns (problems, figures): `problems` lists
    every violated requirement (empty when the device is right), `figures` = {"S12": worst q / t / s gap of a settled
    transform, "flags": unsettled flags on which the two differ, "unsettled": unsettled flags in all}."""
    from amc_lba.sim3_ransac import S3R_DEGENERATE, S3R_NONFINITE
    pairs, corr, hyp = got
    problems, fig = [], {"S12": 0.0, "flags": 0, "unsettled": 0}
    for p, res in enumerate(r64):
        P, D = c.pairs[p], pairs[p]
        flag_ok, transform_ok, sel_ok = ro.settled(res, P, M_GATE, GAP_MIN)
        h0, nh, r0, n = P["hyp0"], P["n_hyp"], P["corr0"], P["n_corr"]
        flags, cnt, S12 = hyp["flags"][h0:h0 + nh], hyp["inliers"][h0:h0 + nh], hyp["S12"][h0:h0 + nh]
        if not ((flags & S3R_DEGENERATE != 0) == res["degenerate"]).all():
            problems.append(f"pair {p}: degenerate flags differ")
        if not ((flags & S3R_NONFINITE != 0) == (res["nonfinite"] & ~res["degenerate"]))[~res["degenerate"]].all():
            problems.append(f"pair {p}: non-finite flags differ")
        unsettled = (~flag_ok).sum(1)
        fig["unsettled"] += int(unsettled.sum())
        off = np.abs(cnt - res["count"])
        if (off > unsettled).any():
            problems.append(f"pair {p}: hyp_inliers off by {off.max()} (unsettled rows {unsettled[off.argmax()]})")
        fig["flags"] += int(off.sum())
        if sel_ok and (D["best_hyp"], D["converged"]) != (res["best_hyp"], res["converged"]):
            problems.append(f"pair {p}: selected {D['best_hyp']} converged {D['converged']}, expected {res['best_hyp']} {res['converged']}")
        if sel_ok and D["best_hyp"] == res["best_hyp"]:
            b = res["best_hyp"]
            row_ok = flag_ok[b] if b >= 0 else np.ones(n, bool)
            if not (corr["inlier"][r0:r0 + n] == res["row_inlier"])[row_ok].all():
                problems.append(f"pair {p}: a settled row's inlier flag differs")
            if b >= 0 and not unsettled[b] and D["n_inliers"] != res["n_inliers"]:
                problems.append(f"pair {p}: n_inliers {D['n_inliers']}, expected {res['n_inliers']}")
            if b >= 0 and D["n_inliers"] != cnt[b]:
                problems.append(f"pair {p}: n_inliers is not the selected hypothesis's count")
            if b >= 0 and not np.array_equal(np.concatenate([D["q"], D["t"], [D["s"]]]), S12[b], equal_nan=True):
                problems.append(f"pair {p}: q, t, s are not the selected hypothesis's")
        gap = s12_gap({"q": S12[:, :4], "t": S12[:, 4:7], "s": S12[:, 7]}, res)[transform_ok]
        if gap.size:
            fig["S12"] = max(fig["S12"], float(gap.max()))
            if not (gap <= 1e-6).all():       # sim3_cases.TOL, relative to max(1, |.|_inf)
                problems.append(f"pair {p}: S12 of a settled transform off by {gap.max():.2e}")
    return problems, fig


def disagreement(res64, res32, rows):
    """largest gate margin (fp64) at which the float32 and fp64 comparisons of one error with its gate disagree"""
    worst = 0.0
    live = ~(res64["degenerate"] | res32["degenerate"])[:, None]
    for e64, e32, g, key in ((res64["err1"], res32["err1"], res64["gate1"], "max_err1"), (res64["err2"], res32["err2"], res64["gate2"], "max_err2")):
        m = np.asarray(rows[key])
        with np.errstate(invalid="ignore"):
            differ = ((e64 < m) != (e32 < m.astype(np.float32))) & live & np.isfinite(g)
        if differ.any():
            worst = max(worst, float(g[differ].max()))
    return worst


def s12_gap(a, b):
    """(q up to sign, t, s) of two hypothesis sets, per hypothesis, relative to max(1, |.|_inf)"""
    with np.errstate(invalid="ignore"):
        gq = np.minimum(np.abs(a["q"] - b["q"]).max(1), np.abs(a["q"] + b["q"]).max(1))
        gt = np.abs(a["t"] - b["t"]).max(1) / np.maximum(1.0, np.abs(b["t"]).max(1))
        gs = np.abs(a["s"] - b["s"]) / np.maximum(1.0, np.abs(b["s"]))
    return np.maximum(np.maximum(gq, gt), gs)
