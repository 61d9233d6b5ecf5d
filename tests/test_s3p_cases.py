"""CPU checks of the Sim3 projection search's cases and of its two numpy restatements (tests/s3p_oracle.py): each named
case has the property it is named for; the loop as written and the route through lba_match_job-shaped jobs agree on every
case and on 200 further seeds; every named case and every GPU seed is settled; each mistake a device could make (no
resolve, quirk (a) or (b) "fixed", the other proj_form) changes a stated, non-zero number of rows of the generated
hypotheses; and the gap to the reference's float32 pose chain is reported and bounded per gate quantity."""
import numpy as np
import pytest

import s3p_cases as sc
import s3p_oracle as so
from amc_lba.sim3_project import S3P_STATUS_NAMES, make_s3p_problem

F = np.float32
LIVE = (0, 1, 2)    # OK, NO_CAND, TOO_FAR: the statuses of a job that passed every gate


def _names(status):
    return [S3P_STATUS_NAMES[int(s)] for s in np.asarray(status).ravel()]


@pytest.mark.parametrize("p", sc.PARAMS, ids=sc.PARAM_IDS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_case_has_its_property_and_both_routes_agree(name, p):
    kfm, hyps, exp = sc.case(name)
    prm = sc.params(p)
    for h in hyps:
        seq = so.sequential(kfm, h, prm)
        jobs, _, _, live = so.by_jobs(kfm, h, prm)
        assert seq.same(jobs)
        if exp.get("only_th", p[0]) != p[0]:
            continue
        st = seq.rows["status"]
        if "live" in exp:
            assert [int(np.isin(st[:, c], LIVE).sum()) for c in range(kfm.n_cam)] == exp["live"]
        if "rounds" in exp:
            assert jobs.poses["rounds"].tolist() == exp["rounds"]
        if "n_matches" in exp:
            assert seq.n_matches == exp["n_matches"]
        if "all_status" in exp:
            assert set(_names(st)) == {exp["all_status"]}
        if "status" in exp:
            assert _names(st) == exp["status"]
        for key in ("feat", "best_dist", "level"):
            if key in exp:
                assert seq.rows[key].ravel().tolist() == exp[key]
        if "n_feat_cam" in exp:
            assert np.bincount(kfm.feats["cam"]).max() == exp["n_feat_cam"]


def test_z_zero_projects_to_infinity_not_nan():
    kfm, hyps, _ = sc.case("z_zero_and_behind")
    for form in (0, 1):
        r = so.sequential(kfm, hyps[0], sc.params((8, 1.5, form))).rows
        assert np.isinf(r["x"][:2, 0]).all() and r["x"][0, 0] > 0 > r["x"][1, 0]


@pytest.mark.parametrize("seed", range(200))
def test_both_routes_agree_on_further_seeds(seed):
    kfm, hyps = make_s3p_problem(n_cam=1 + seed % 4, n_feat=60, n_hyp=1, n_points=80, seed=1000 + seed)
    prm = sc.params(sc.PARAMS[seed % len(sc.PARAMS)])
    assert so.sequential(kfm, hyps[0], prm).same(so.by_jobs(kfm, hyps[0], prm)[0])


def _all_problems():
    for name in sc.NAMES:
        k, h, _ = sc.case(name)
        yield name, k, h
    for seed in sc.GPU_SEEDS:
        k, h = sc.gpu_problem(seed)
        yield "gpu_seed_%d" % seed, k, h
    k, h = sc.batch_33()
    yield "batch_33", k, h


def test_every_named_case_and_gpu_seed_is_settled():
    for name, k, hyps in _all_problems():
        if not k.kf[0]["has_prev"]:
            continue
        for i, h in enumerate(hyps):
            assert sc.pose_settled(k, h), (name, i)
            for p in (sc.PARAMS[0], sc.PARAMS[1]):       # the quotient does not depend on th or the ratio
                assert sc.level_settled(so.sequential(k, h, sc.params(p)).quot), (name, i)
    assert len(sc.batch_33()[1]) == 33


def _changed(a, b):
    return int(((a.rows["status"] != b.rows["status"]) | (a.rows["feat"] != b.rows["feat"])).sum())


def test_each_mistake_changes_rows_of_the_generated_hypotheses():
    """a device without the resolve, with quirk (a) or (b) "fixed", or with the other proj_form would each fail the GPU
    test: on the GPU seeds each changes this many (status, feat) rows, or x bits for the form"""
    counts = dict(no_resolve=0, fix_a=0, fix_b=0)
    form_bits = 0
    for seed in sc.GPU_SEEDS:
        k, hyps = sc.gpu_problem(seed)
        k.kcams["ow"][:, 2] += F(0.5)     # (a) only shows where the map's centre is off the corrected one
        for h in hyps:
            prm = sc.params(sc.PARAMS[0])
            ref = so.sequential(k, h, prm)
            for v in counts:
                counts[v] += _changed(ref, so.sequential(k, h, prm, variant=v))
            other = so.sequential(k, h, sc.params(sc.PARAMS[1]))
            reached = np.isin(ref.rows["status"], LIVE)
            form_bits += int((ref.rows["x"].view(np.uint32) != other.rows["x"].view(np.uint32))[reached].sum())
    print("rows changed by each mistake on the GPU seeds:", counts, "x bits changed by the other proj_form:", form_bits)
    assert all(v > 0 for v in counts.values()) and form_bits > 0, (counts, form_bits)


def test_gap_to_the_float32_chain_is_bounded_per_gate_quantity():
    """The reference finishes the pose chain in SE3f.  Reported: the largest difference of x, y in pixels and of each
    gate quantity between this function's Tcw (fp64, rounded once) and a float32 chain.  Asserted (the per-quantity rule
    of DESIGN.md §7 item 10): a job's status differs only where one of its gate quantities (depth, the four image
    margins) lies within 4 x that quantity's largest measured difference of its gate.  The distance and viewing gates
    and PredictScale do not read Tcw at all (quirk (a): they use the map's camera centre), so they cannot differ."""
    worst = dict(z=0.0, u=0.0, v=0.0)
    rows = []
    for seed in sc.GPU_SEEDS:
        k, hyps = sc.gpu_problem(seed)
        for h in hyps:
            prm = sc.params(sc.PARAMS[0])
            ours = so.sequential(k, h, prm)
            t32 = so.pose_float32_chain(k, h)
            theirs = so.sequential(k, h, prm, tcw=t32)
            for p, P in enumerate(h.points):
                for c in range(k.n_cam):
                    if P["skip"]:
                        continue
                    za, ua, va = so.gate_quantities(ours.poses["tcw"][c], k.kcams[c], P, prm)
                    zb, ub, vb = so.gate_quantities(t32[c], k.kcams[c], P, prm)
                    differs = ours.rows["status"][p, c] in LIVE and theirs.rows["status"][p, c] not in LIVE or \
                        ours.rows["status"][p, c] not in LIVE and theirs.rows["status"][p, c] in LIVE
                    if za > 0.1 and zb > 0.1:        # pixels only mean something in front of the camera
                        inside = 0 <= ua < 640 and 0 <= va < 480
                        if inside:
                            worst["u"], worst["v"] = max(worst["u"], abs(ua - ub)), max(worst["v"], abs(va - vb))
                        worst["z"] = max(worst["z"], abs(za - zb))
                    if differs:
                        C = k.kcams[c]
                        rows.append((za, ua - C["min_x"], C["max_x"] - ua, va - C["min_y"], C["max_y"] - va))
    print("gap to the float32 chain: x %.3e px, y %.3e px, depth %.3e; jobs whose gate status differs: %d"
          % (worst["u"], worst["v"], worst["z"], len(rows)))
    assert worst["u"] < 0.05 and worst["v"] < 0.05      # float32 poses: a few 1e-3 px at these depths
    for za, l, r, t, b in rows:
        near = abs(za) <= 4 * worst["z"] or min(abs(l), abs(r)) <= 4 * worst["u"] or min(abs(t), abs(b)) <= 4 * worst["v"]
        assert near, (za, l, r, t, b)
