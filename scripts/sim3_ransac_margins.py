"""The margins behind the tests of lba_sim3_ransac, written to profiles/sim3_ransac_margins.log.

CPU part (always): over the named cases of tests/sim3_ransac_cases.py and six seeds of the 300-hypothesis set-up
(100 rows, 4 cameras, 30 % outliers), the largest gate margin at which a float32 and an fp64 comparison of one error
with its gate disagree (M_GATE is 4 x that), the share of flags inside M_GATE, the smallest eigen-gap, and the float32 /
fp64 distance of S12.  GPU part (--gpu): the device against the fp64 restatement on the named cases.

    python scripts/sim3_ransac_margins.py [--gpu] [--out profiles/sim3_ransac_margins.log]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "amc-slam_amd"), os.path.join(ROOT, "tests")]
import sim3_ransac_cases as rc  # noqa: E402
import sim3_ransac_oracle as ro  # noqa: E402

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sim3_ransac_margins.log")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def measure(label, c):
    r64, r32 = c.oracle(np.float64), c.oracle(np.float32)
    worst = near = flags = 0
    gap_min, s12 = np.inf, 0.0
    for p, (a, b) in enumerate(zip(r64, r32)):
        worst = max(worst, rc.disagreement(a, b, c.pair_inputs(p)[1]))
        flag_ok, transform_ok, _ = ro.settled(a, c.pairs[p], rc.M_GATE, rc.GAP_MIN)
        near += int((~flag_ok).sum())
        flags += flag_ok.size
        live = ~(a["degenerate"] | a["nonfinite"])
        if live.any():
            gap_min = min(gap_min, float(a["gap"][live].min()))
        g = rc.s12_gap(b, a)[transform_ok]
        if g.size:
            s12 = max(s12, float(g.max()))
    say(f"{label:28s} flags {flags:6d}  inside M_GATE {near:3d}  largest disagreeing margin {worst:.3e}  smallest gap {gap_min:.2e}  "
        f"float32 vs fp64 S12 {s12:.2e}")
    return worst, near, flags, s12


say(f"lba_sim3_ransac: float32 (reference-faithful) against fp64 (what the device is held to), numpy restatements; M_GATE = {rc.M_GATE:.1e}")
tot = np.zeros(4)
for name in rc.NAMES:
    w = measure(name, rc.case(name)[0])
    tot = np.array([max(tot[0], w[0]), tot[1] + w[1], tot[2] + w[2], max(tot[3], w[3])])
for seed in range(6):
    w = measure(f"300 hypotheses, seed {seed}", rc._gen(n_corr=100, n_hyp=300, seed=seed))
    tot = np.array([max(tot[0], w[0]), tot[1] + w[1], tot[2] + w[2], max(tot[3], w[3])])
say(f"all: largest gate margin with a float32 / fp64 disagreement {tot[0]:.3e}, x 4 = {4 * tot[0]:.3e} (M_GATE {rc.M_GATE:.1e}); "
    f"{int(tot[1])} of {int(tot[2])} flags inside M_GATE ({tot[1] / tot[2]:.1e}); float32 vs fp64 S12 at most {tot[3]:.2e} "
    f"(S12_F32_BOUND {rc.S12_F32_BOUND:.0e})")
if tot[0] == 0:
    say("no disagreement at all: 4 x the measurement is 0, and M_GATE rests on the number formats instead (float32's 6e-8 on "
        "image coordinates up to 1000 px through 8 operations = 5e-4 px, on 3 px at the gate of 9: 3e-4 relative, rounded up)")

if "--gpu" in sys.argv:
    from amc_lba.track import Tracker, track_config
    t = Tracker(track_config())
    say("device against the fp64 restatement (tolerance on S12: 1e-6 relative to max(1, |.|_inf))")
    worst, diff, uns, bad = 0.0, 0, 0, 0
    for name in rc.NAMES:
        c, r64, _ = rc.case(name)
        problems, fig = rc.device_gaps(c, r64, rc.run_device(t, c))
        say(f"{name:28s} S12 {fig['S12']:.2e}  count differences on unsettled flags {fig['flags']} of {fig['unsettled']}  {'; '.join(problems) or 'ok'}")
        worst, diff, uns, bad = max(worst, fig["S12"]), diff + fig["flags"], uns + fig["unsettled"], bad + len(problems)
    say(f"all: S12 of settled transforms within {worst:.2e}; {diff} count differences on {uns} unsettled flags; {bad} problems")
    t.close()

with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
