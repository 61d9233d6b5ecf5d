"""Measures what the tests of lba_match_fuse's split rest on and writes profiles/fuse_margins.log.  CPU only.

  * the level margin: over every named case (tests/fuse_cases.py), the GPU seeds and 20 further seeds, the smallest
    distance of a PredictScale quotient from an integer, against M_LEVEL (tests/s3p_cases.py: the same function);
  * the redo share: for SearchInNeighbors' two phases over 20 targets and SearchAndFuse with its replace loop on
    generated maps (tests/test_fuse_walk.py's own runs and 6 further seeds each), the jobs fuse_walk redoes on the CPU
    as a share of the rows with status OK or TOO_FAR, against the cap of 10 %, and the rows it goes on to use that an
    IsInKFCamera applied up front would not have.

    python scripts/fuse_margins.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("tests", "oracle", "amc-slam_amd"):
    sys.path.insert(0, os.path.join(ROOT, d))

import fuse_cases as fc  # noqa: E402
import fuse_oracle as fo  # noqa: E402
import test_fuse_walk as tw  # noqa: E402
from amc_lba.fuse import FUSE_KF, make_fuse_problem  # noqa: E402


def main():
    lines, worst = [], np.inf
    for name in fc.NAMES:
        c = fc.case(name)
        qs = [fo.sequential(c.targets[t], c.points[p0:p0 + n], FUSE_KF, fc.TH[FUSE_KF])[1] for t, p0, n in c.searches]
        q = np.concatenate([x.ravel() for x in qs]) if qs else np.zeros(0)
        q = q[np.isfinite(q)]
        m = float(np.abs(q - np.round(q)).min()) if len(q) else np.inf
        worst = min(worst, m)
        lines.append("%-24s level margin %.3e" % (name, m))
    for seed in range(20):
        prob = fc.gpu_problem(seed) if seed in fc.GPU_SEEDS else make_fuse_problem(n_kf=21, n_cam=4, n_feat=120, n_points=260, seed=seed)
        P = prob.points(np.arange(prob.n_ids))
        q = np.concatenate([fo.sequential(tg, P, FUSE_KF, fc.TH[FUSE_KF])[1].ravel() for tg in prob.targets[:6]])
        q = q[np.isfinite(q)]
        m = float(np.abs(q - np.round(q)).min())
        worst = min(worst, m)
        lines.append("%-24s level margin %.3e" % ("seed_%d%s" % (seed, " (GPU)" if seed in fc.GPU_SEEDS else ""), m))
    head = ["smallest distance of a PredictScale quotient from an integer: %.3e (M_LEVEL = %.1e)" % (worst, fc.M_LEVEL), ""]
    shares = []
    for seed in range(8):
        prob = make_fuse_problem(n_kf=21, n_cam=4, n_feat=100, n_points=220, seed=seed)
        t = tw.Tally()
        tw.search_in_neighbors(prob, 0, list(range(1, 21)), t)
        shares.append(t.redone / max(1, t.decided))
        lines.append("SearchInNeighbors seed %d%s: %d redone of %d OK / TOO_FAR rows (%.2f %%), %d used rows IsInKFCamera "
                     "would have dropped" % (seed, " (test)" if seed < 2 else "", t.redone, t.decided, 100 * shares[-1],
                                             t.in_kf_rows_used))
    for seed in range(8):
        prob = make_fuse_problem(n_kf=12, n_cam=4, n_feat=100, n_points=220, seed=100 + seed, duplicates=0.08)
        t = tw.Tally()
        tw.search_and_fuse(prob, list(range(3, 12)), tw.loop_list(prob, fo.ToyMap.from_problem(prob), [0, 1, 2]), t)
        shares.append(t.redone / max(1, t.decided))
        lines.append("SearchAndFuse seed %d%s: %d redone of %d OK / TOO_FAR rows (%.2f %%)"
                     % (100 + seed, " (test)" if seed < 2 else "", t.redone, t.decided, 100 * shares[-1]))
    head.insert(1, "largest redo share on a generated problem: %.2f %% (cap %.0f %%)" % (100 * max(shares), 100 * tw.CAP))
    text = "\n".join(head + lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "fuse_margins.log"), "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
