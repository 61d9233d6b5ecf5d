"""Counts what the tests of lba_mappoint_refresh rest on and writes profiles/mappoint_margins.log.  CPU only.

For each of six mistakes (tests/mp_oracle.py: the upper median, ties to the last row, bad keyframes skipped in the
normal, a pairwise sum, a multiplication by 1 / r, a contracted fma in the squared norm) the points of the generated
batches (tests/mp_cases.py, the seeds of tests/test_mp_cases.py) whose refreshed record it would change.  Each must
change at least one, or the generator is too tame; the same counts over the GPU test's batches follow.

    python scripts/mappoint_margins.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("tests", "oracle", "amc-slam_amd"):
    sys.path.insert(0, os.path.join(ROOT, d))

import mp_cases as mc  # noqa: E402
import mp_oracle as mo  # noqa: E402
import test_mp_cases as tc  # noqa: E402


def main():
    counts, total = tc.mistake_counts()
    lines = ["points whose refreshed record a mistake changes, over the %d points of seeds %d .. %d:"
             % (total, tc.MISTAKE_SEEDS[0], tc.MISTAKE_SEEDS[-1])]
    lines += ["  %-20s %5d  (%.1f %%)" % (m, counts[m], 100.0 * counts[m] / total) for m in mo.MISTAKES]
    p = mc.gpu_problem(mc.GPU_SEEDS[0])
    sub = p.points[::8]
    right = mo.refresh_batch(sub, p.obs, p.K, p.kf_bad, form=mo.refresh_loops)
    lines += ["", "the same over every eighth point (%d) of the GPU test's batch of seed %d:" % (len(sub), mc.GPU_SEEDS[0])]
    for m in mo.MISTAKES:
        wrong = mo.refresh_batch(sub, p.obs, p.K, p.kf_bad, form=mo.refresh_loops, **{m: True})
        n = sum(mo.diff_fields(wrong[i], right[i]) != [] for i in range(len(sub)))
        lines.append("  %-20s %5d  (%.1f %%)" % (m, n, 100.0 * n / len(sub)))
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "mappoint_margins.log"), "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
