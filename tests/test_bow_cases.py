"""The two restatements of SearchByBoW (tests/bow_oracle.py) agree on every named case (tests/bow_cases.py), in both
overloads, and on 200 further generator seeds; every case has its property; idx2 is unique among the accepted rows of a
pair; and the variants a wrong device would compute (no matched flag, ties to the last position, the ratio product in
double) each change at least 20 rows of the generated pairs the GPU test uses.  No GPU."""
import numpy as np
import pytest

import bow_cases as bc
import bow_oracle as bo
from amc_lba.abi import BOW_ROW_DTYPE
from amc_lba.bow import BOW_OK, BOW_ROT, bow_matches


def unique_idx2(r):
    took = r.idx2[(r.status == bo.OK) | (r.status == bo.ROT)]
    return len(np.unique(took)) == len(took) and (took >= 0).all()


@pytest.mark.parametrize("mode", bc.MODES, ids=bc.MODE_NAMES.get)
@pytest.mark.parametrize("name", bc.NAMES)
def test_case_restatements_agree_and_property_holds(name, mode):
    c, seq = bc.case(name, mode)
    for j, s in zip(bo.jobs_of(c), seq):
        assert bo.same(s, bo.by_node(j))
        assert unique_idx2(s)
        assert s.n_matches == (s.status == bo.OK).sum()
        ran = np.isin(s.status, (bo.OK, bo.NO_CAND, bo.RATIO, bo.ROT))
        assert ((s.idx2[~ran] == -1) & (s.dist[~ran] == 256) & (s.dist2[~ran] == 256)).all()
        assert (s.dist <= s.dist2).all() and ((s.idx2 == -1) == (s.dist == 256)).all()
    c.prop(c, seq)


def test_restatements_agree_on_200_seeds():
    total = 0
    for seed in range(200):
        mode = bc.MODES[seed % 2]
        prm = dict(nn_ratio=(0.9, 0.7, 0.6, 0.75)[seed % 4], check_orientation=seed % 3 != 0, th_low=(50, 50, 30)[seed % 3])
        c = bc.generated(1 + seed % 2, 1000 + seed, mode, prm, n_feat=60 + seed % 50, n_nodes=3 + seed % 5, cluster=1 + seed % 5)
        for j in bo.jobs_of(c):
            s = bo.sequential(j)
            assert bo.same(s, bo.by_node(j)), seed
            assert unique_idx2(s), seed
            total += s.n_matches
    assert total > 2000


def test_variants_bite_on_the_generated_pairs():
    """computed by the restatement alone, on the pairs tests/test_gpu_bow.py::test_variants_on_generated_pairs uses"""
    for mode in bc.MODES:
        c = bc.generated(*bc.VARIANT_PAIRS, mode, dict(nn_ratio=0.6), **bc.VARIANT_GEN)
        n = dict(no_flag=0, tie_last=0, ratio_double=0)
        for j in bo.jobs_of(c):
            s = bo.sequential(j)
            n["no_flag"] += bo.rows_differing(s, bo.sequential(j, flag=False))
            n["tie_last"] += bo.rows_differing(s, bo.sequential(j, tie="last"))
            n["ratio_double"] += bo.rows_differing(s, bo.sequential(j, ratio_double=True))
        print(f"{bc.MODE_NAMES[mode]}: rows changed by the variants {n}")
        assert all(v >= 20 for v in n.values()), n


def test_float_ratio_pairs_counted():
    """the (b1, b2) at which the float product and the product in double decide differently: none at 0.9, 0.7 and
    0.75, 33 at 0.6f, 51 at 0.8f"""
    b1, b2 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    for ratio, want in ((0.9, 0), (0.7, 0), (0.75, 0), (0.6, 33), (0.8, 51)):
        r = np.float32(ratio)
        f = b1.astype(np.float32) < r * b2.astype(np.float32)
        d = b1.astype(np.float64) < np.float64(r) * b2.astype(np.float64)
        assert int((f != d).sum()) == want, (ratio, int((f != d).sum()))


def test_bow_matches_lists_the_ok_rows():
    rows = np.zeros(5, BOW_ROW_DTYPE)
    rows["status"], rows["idx2"] = (BOW_OK, 3, BOW_ROT, BOW_OK, 1), (4, -1, 2, 0, -1)
    assert bow_matches(None, rows).tolist() == [[0, 4], [3, 0]]
