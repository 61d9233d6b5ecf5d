"""Measures the two settledness margins of the Sim3 projection search's tests and writes profiles/sim3_project_margins.log.

Over every named case (tests/s3p_cases.py), the generated GPU seeds and 40 further seeds: the largest fp64
difference (relative to the entry's scale: 1 for a rotation entry, max(1, |t|) for a translation entry) between the pose chain of csrc/lba_s3p_math.hpp built for the host and tests/s3p_oracle.py's (numpy around the
C oracle's QueryPose), and the largest difference of PredictScale's quotient between the two.  M = max(1e-12, 64 x that).
Then the settledness of every case and seed under these margins.  CPU only.

    python scripts/s3p_margins.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("tests", "oracle", "amc-slam_amd"):
    sys.path.insert(0, os.path.join(ROOT, d))

import s3p_cases as sc  # noqa: E402
import s3p_oracle as so  # noqa: E402
import test_s3p_host as th  # noqa: E402


def problems():
    for name in sc.NAMES:
        k, h, _ = sc.case(name)
        yield name, k, h
    k, h = sc.batch_33()
    yield "batch_33", k, h
    for seed in range(40):
        k, h = sc.gpu_problem(seed)
        yield "seed_%d%s" % (seed, " (GPU)" if seed in sc.GPU_SEEDS else ""), k, h


def main():
    L = th.load_harness()
    lines, worst_pose, worst_q = [], 0.0, 0.0
    settled = []
    for name, k, hyps in problems():
        if not k.kf[0]["has_prev"]:
            continue
        dp = dq = 0.0
        mp, mq = np.inf, np.inf
        for h in hyps:
            want = so.pose_f64(k, h)
            dp = max(dp, float(so.pose_diff(th.host_pose(L, k, h), want).max()))
            mp = min(mp, float(so.pose_margin(want).min()))
            res = so.sequential(k, h, sc.params(sc.PARAMS[0]))
            for (p, c), q in np.ndenumerate(res.quot):
                if not np.isfinite(q):
                    continue
                P, C = h.points[p], k.kcams[c]
                o = P["pos"] - C["ow"]
                dist = np.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
                dq = max(dq, abs(L.sh_quotient(P["max_distance"], dist, k.kf[0]["log_scale_factor"]) - q))
                mq = min(mq, abs(q - np.round(q)))
        worst_pose, worst_q = max(worst_pose, dp), max(worst_q, dq)
        settled.append((name, mp, mq))
        lines.append("%-28s pose diff %.3e  quotient diff %.3e  | pose margin %.3e  level margin %.3e" % (name, dp, dq, mp, mq))
    m_pose, m_level = max(1e-12, 64 * worst_pose), max(1e-12, 64 * worst_q)
    head = ["largest fp64 difference of a Tcw entry relative to its scale, host header vs numpy restatement: %.3e" % worst_pose,
            "largest difference of PredictScale's quotient: %.3e" % worst_q,
            "M_POSE  = max(1e-12, 64 x %.3e) = %.3e" % (worst_pose, m_pose),
            "M_LEVEL = max(1e-12, 64 x %.3e) = %.3e" % (worst_q, m_level),
            "fixed in tests/s3p_cases.py: M_POSE = %.3e, M_LEVEL = %.3e" % (sc.M_POSE, sc.M_LEVEL),
            "unsettled under the fixed margins: " + (", ".join(n for n, a, b in settled if a <= sc.M_POSE or b <= sc.M_LEVEL) or "none"), ""]
    text = "\n".join(head + lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "sim3_project_margins.log"), "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
