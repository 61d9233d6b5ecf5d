"""The named cases of lba_mappoint_refresh (tests/mp_cases.py) on the two numpy restatements (tests/mp_oracle.py): each
case shows its property, and the loops and the vectorised form agree in every field (float bits, a NaN matching a NaN)
on the cases and on 200 generated batches.  Six mistakes are counted on the generated batches: each must change at
least one point, or the generator is too tame (scripts/mappoint_margins.py writes the counts to
profiles/mappoint_margins.log).  A permuted list changes the normal's bits, so the order is pinned."""
import numpy as np
import pytest

import mp_cases as mc
import mp_oracle as mo

CHUNK = 20
MISTAKE_SEEDS = range(40)


def both_forms(points, obs, K, kf_bad, label):
    a = mo.refresh_batch(points, obs, K, kf_bad, form=mo.refresh_loops)
    b = mo.refresh_batch(points, obs, K, kf_bad, form=mo.refresh_vec)
    for i in range(len(points)):
        assert mo.diff_fields(a[i], b[i]) == [], (label, i, mo.diff_fields(a[i], b[i]))
    return a


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_property_and_the_two_restatements_agree(name):
    c = mc.case(name)
    R = both_forms(c.points, c.obs, c.K, c.kf_bad, name)
    assert mo.diff_fields(R, mc.reference(name)) == []
    if c.check is not None:
        c.check(R)
    # what the reference does not write comes back as given
    for i, P in enumerate(c.points):
        for f in ("pos", "ref_kf", "obs0", "n_obs", "bad", "ops"):
            assert R[i][f].tobytes() == P[f].tobytes()
        if R[i]["status"] != mc.MP_OK:
            for f in ("normal", "min_distance", "max_distance", "desc"):
                assert R[i][f].tobytes() == P[f].tobytes(), (name, f)


@pytest.mark.parametrize("first", range(0, len(mc.SEEDS), CHUNK))
def test_generated_batches_agree(first):
    for seed in range(first, first + CHUNK):
        p = mc.problem(seed)
        both_forms(p.points, p.obs, p.K, p.kf_bad, seed)


def test_generated_batches_are_not_tame():
    """statuses, both operations, bad keyframes among the observations, several cameras of the reference keyframe, no
    reference keyframe, and lists longer than a wave all occur"""
    seen = dict(bad=0, empty=0, ops1=0, ops2=0, bad_obs=0, ref_multi=0, no_ref=0, long=0)
    for seed in range(12):
        p = mc.problem(seed)
        seen["bad"] += int((p.points["bad"] != 0).sum())
        seen["empty"] += int((p.points["n_obs"] == 0).sum())
        seen["ops1"] += int((p.points["ops"] == 1).sum())
        seen["ops2"] += int((p.points["ops"] == 2).sum())
        seen["long"] += int((p.points["n_obs"] > 64).sum())
        for P in p.points:
            L = p.obs[int(P["obs0"]):int(P["obs0"]) + int(P["n_obs"])]
            seen["bad_obs"] += int(p.kf_bad[L["kf"]].any())
            seen["ref_multi"] += int((L["kf"] == P["ref_kf"]).sum() > 1)
            seen["no_ref"] += int(len(L) > 0 and P["ref_kf"] == -1)
    assert all(v > 0 for v in seen.values()), seen


def mistake_counts(seeds=MISTAKE_SEEDS):
    """per mistake the points of the generated batches whose refreshed record it changes, and the points in all"""
    counts, total = {m: 0 for m in mo.MISTAKES}, 0
    for seed in seeds:
        p = mc.problem(seed)
        right = mo.refresh_batch(p.points, p.obs, p.K, p.kf_bad, form=mo.refresh_loops)
        total += len(right)
        for m in mo.MISTAKES:
            wrong = mo.refresh_batch(p.points, p.obs, p.K, p.kf_bad, form=mo.refresh_loops, **{m: True})
            counts[m] += sum(mo.diff_fields(wrong[i], right[i]) != [] for i in range(len(right)))
    return counts, total


def test_every_mistake_changes_a_point():
    counts, total = mistake_counts()
    print("mistakes over %d points: %s" % (total, counts))
    assert all(v >= 1 for v in counts.values()), counts


def test_a_permuted_list_changes_the_normals_bits():
    _, _, a, b = mc.order_matters()
    assert a["normal"].tobytes() != b["normal"].tobytes()
    assert np.allclose(a["normal"], b["normal"], rtol=1e-5, atol=1e-6) and int(a["n"]) == int(b["n"])
