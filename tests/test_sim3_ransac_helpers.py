"""The caller-side restatements of amc_lba.sim3_ransac on plain arrays: sim3_ransac_rows (the constructor's filtering,
src/Sim3Solver.cc:85-147, with the truncated gates of quirk a), ransac_max_iterations (SetRansacParameters, :155-179),
draw_triples (:277-291) and seed_sim3_pairs (LoopClosing.cc:576)."""
import math

import numpy as np
import pytest

from amc_lba.sim3 import SIM3_PAIR_DTYPE
from amc_lba.sim3_ransac import (S3R_PAIR_DTYPE, draw_triples, make_sim3_ransac_pairs, max_error, ransac_max_iterations,
                                 seed_sim3_pairs, sim3_ransac_rows)


def test_gates_are_truncated_to_integers():
    sigma2 = np.float32(1.2) ** (2 * np.arange(8))             # mvLevelSigma2 of a 1.2 pyramid, float
    got = max_error(sigma2)
    assert got[0] == 9 and got[1] == 13
    assert (got == np.floor(9.210 * sigma2.astype(np.float64))).all() and (got == np.round(got)).all()
    assert (got <= 9.210 * sigma2).all() and (got > 9.210 * sigma2 - 1).all()


def test_rows_follow_the_constructor():
    N = 12
    rng = np.random.default_rng(0)
    match = np.ones(N, bool); has1 = np.ones(N, bool); bad1 = np.zeros(N, bool); bad2 = np.zeros(N, bool)
    index1 = np.arange(N); index2 = np.arange(N) + 100
    match[1] = False          # vpMatched12[i1] == NULL
    has1[2] = False           # !pMP1
    bad1[3] = True            # pMP1->isBad()
    bad2[4] = True            # pMP2->isBad()
    index1[5] = -1            # indexKF1 < 0
    index2[6] = -1            # indexKF2 < 0: no camera of the matched keyframe has the point
    cam1, cam2 = rng.integers(0, 4, N), rng.integers(0, 4, N)
    X1, X2 = rng.normal(size=(N, 3)) * 10, rng.normal(size=(N, 3)) * 10
    s1 = (np.float32(1.2) ** (2 * rng.integers(0, 8, N))).astype(np.float32)
    s2 = (np.float32(1.2) ** (2 * rng.integers(0, 8, N))).astype(np.float32)
    rows, idx = sim3_ransac_rows(match, has1, bad1, bad2, index1, index2, cam1, cam2, X1, X2, s1, s2)
    assert list(idx) == [0, 7, 8, 9, 10, 11]                   # mvnIndices1
    assert (rows["cam1"] == cam1[idx]).all() and (rows["cam2"] == cam2[idx]).all()
    assert (rows["X1b"] == X1[idx].astype(np.float32)).all() and (rows["X2b"] == X2[idx].astype(np.float32)).all()
    assert (rows["max_err1"] == np.floor(9.210 * s1[idx].astype(np.float64))).all()
    assert (rows["max_err2"] == np.floor(9.210 * s2[idx].astype(np.float64))).all()
    assert not rows["inlier"].any()
    none, idx0 = sim3_ransac_rows(np.zeros(N, bool), has1, bad1, bad2, index1, index2, cam1, cam2, X1, X2, s1, s2)
    assert len(none) == 0 and len(idx0) == 0


def _reference_iterations(N, prob, min_inliers, max_its):
    if min_inliers == N:
        n = 1
    else:
        eps = np.float32(np.float32(min_inliers) / np.float32(N))           # float epsilon = (float)minInliers / N
        n = math.ceil(math.log(1 - prob) / math.log(1 - float(eps) ** 3))   # pow, log: double
    return max(1, min(n, max_its))


def test_max_iterations():
    assert ransac_max_iterations(20, 0.99, 20, 300) == 1                    # mRansacMinInliers == N
    assert ransac_max_iterations(30, 0.99, 15, 300) == 35                   # epsilon 0.5: ceil(log 0.01 / log 0.875)
    assert ransac_max_iterations(100, 0.99, 15, 300) == 300                 # 1363 capped by maxIterations
    assert ransac_max_iterations(16, 0.99, 15, 300) == 3
    assert ransac_max_iterations(16, 0.5, 15, 300) == 1                     # ceil(0.42) = 1
    assert ransac_max_iterations(15, 0.99, 20, 300) == 1                    # never reached (N < minInliers exits): max(1, .)
    for N in range(15, 200):
        for mi in (15, 20):
            if N >= mi:
                assert ransac_max_iterations(N, 0.99, mi, 300) == _reference_iterations(N, 0.99, mi, 300), (N, mi)
    # the float epsilon decides: where the double quotient would give another count
    differs = [(N, mi) for N in range(16, 400) for mi in range(3, 16) if N > mi and
               math.ceil(math.log(0.01) / math.log(1 - (mi / N) ** 3)) != _reference_iterations(N, 0.99, mi, 10**9)]
    for N, mi in differs[:5]:
        assert ransac_max_iterations(N, 0.99, mi, 10**9) == _reference_iterations(N, 0.99, mi, 10**9)
    print(f"{len(differs)} (N, minInliers) pairs where the float epsilon changes the count, e.g. {differs[:3]}")


class _Scripted:
    """a generator whose integers() returns a scripted sequence and records the bounds it was asked for"""
    def __init__(self, values):
        self.values, self.asked = list(values), []

    def integers(self, lo, hi):
        self.asked.append((lo, hi))
        return self.values.pop(0)


def test_draw_triples_swaps_with_the_back():
    # N = 5: draw slot 0 -> row 0, slot 0 now holds row 4; draw slot 0 again -> row 4, slot 0 holds row 3; slot 2 -> row 2
    rng = _Scripted([0, 0, 2, 4, 3, 0])
    tri = draw_triples(5, 2, rng)
    assert tri.tolist() == [[0, 4, 2], [4, 3, 0]]
    assert rng.asked == [(0, 5), (0, 4), (0, 3)] * 2            # RandomInt(0, size - 1), inclusive
    tri = draw_triples(40, 500, np.random.default_rng(1))
    assert tri.shape == (500, 3) and tri.dtype == np.int32 and tri.min() == 0 and tri.max() == 39
    assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 1] != tri[:, 2]).all() and (tri[:, 0] != tri[:, 2]).all()
    assert len(draw_triples(3, 0, np.random.default_rng(1))) == 0
    with pytest.raises(ValueError):
        draw_triples(2, 1, np.random.default_rng(1))


def test_seed_sim3_pairs():
    rp = np.zeros(3, S3R_PAIR_DTYPE)
    rp["q"], rp["t"], rp["s"] = [(0, 0, 0.6, 0.8)] * 3, [(1, 2, 3)] * 3, (1.1, 1.2, 1.3)
    rp["best_hyp"], rp["converged"] = (4, -1, 0), (1, 0, 0)
    sp = np.zeros(3, SIM3_PAIR_DTYPE)
    sp["q"], sp["s"], sp["th2"] = (0, 0, 0, 1), 1.0, 10.0
    conv = seed_sim3_pairs(rp, sp)
    assert conv.tolist() == [True, False, False]
    assert sp["s"].tolist() == [1.1, 1.0, 1.3] and sp["q"][1].tolist() == [0, 0, 0, 1] and sp["t"][2].tolist() == [1, 2, 3]
    assert (sp["th2"] == 10.0).all()
    with pytest.raises(ValueError):
        seed_sim3_pairs(rp[:2], sp)


def test_generator_is_reproducible_and_float_valued():
    a = make_sim3_ransac_pairs(n_pairs=2, n_corr=30, n_hyp=10, seed=3)
    b = make_sim3_ransac_pairs(n_pairs=2, n_corr=30, n_hyp=10, seed=3)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    pairs, corr, samples, cams, truth = a
    assert (corr["X1b"] == corr["X1b"].astype(np.float32)).all() and (corr["X2b"] == corr["X2b"].astype(np.float32)).all()
    assert set(corr["max_err1"]) <= {9.0, 13.0} and samples.shape == (20, 3) and len(cams) == 16
    assert 0 < truth["gross"].sum() < 30 and len(truth["sim3_corr"]) == 60
