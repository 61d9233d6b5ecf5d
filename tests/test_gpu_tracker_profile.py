"""The event brackets of the tracker's four calls on the pinned arena (lba_sim3_profile, lba_sim3_ransac_profile,
lba_triangulate_profile, lba_match_profile; Tracker.*_kernel_ms): they share one set of events on the handle, two
marks for three of them and three for the matcher, so each is switched on alone while all four calls run.

Per entry point: -1 before its first timed call; with its bracket on and the others off only its value changes, to a
finite time >= 0, and every call's outputs are bitwise those of the untimed calls; switched off again, a further call
leaves the stored value as it was."""
import functools
import math

import numpy as np
import pytest

import match_cases as mc
import match_oracle as mo
from amc_lba.match import MATCH_OK, match_params, pack_searches
from amc_lba.sim3 import make_sim3_pairs
from amc_lba.sim3_ransac import make_sim3_ransac_pairs
from amc_lba.track import Tracker, track_config
from amc_lba.triangulate import make_tri_pairs

CALLS = ("sim3", "sim3_ransac", "triangulate", "match")
N_MS = {"sim3": 1, "sim3_ransac": 1, "triangulate": 1, "match": 2}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    if name == "sim3":
        return make_sim3_pairs(n_pairs=2, n_corr=30)[:3]
    if name == "sim3_ransac":
        return make_sim3_ransac_pairs(n_pairs=2, n_corr=20, n_hyp=40, min_inliers=6)[:4]
    if name == "triangulate":
        return make_tri_pairs(n_pairs=1, n_rows=70)[:4]           # two chunks: 64 + 6 rows
    return {m: mc.small_batch(m, 2) for m in mc.BOTH}              # two searches, 1 and 2 cameras


def _run(t, name):
    """the call on fresh copies of its inputs; every output array as bytes"""
    a = _inputs(name)
    if name == "sim3":
        out = t.sim3_optimize(a[0].copy(), a[1].copy(), a[2], 4)
    elif name == "sim3_ransac":
        p, c, hyp = t.sim3_ransac(a[0].copy(), a[1].copy(), a[2], a[3], 4)
        out = [p, c] + [hyp[k] for k in sorted(hyp)]
    elif name == "triangulate":
        out = t.triangulate(a[0].copy(), a[1].copy(), a[2], a[3], 4)
    else:
        out = []
        for mode in mc.BOTH:
            S, cams, cs, cf, feats, jobs = pack_searches(a[mode])
            out += t.match_project(S, cams, cs, cf, feats, jobs, match_params(mode, 1))
    return [np.ascontiguousarray(o).tobytes() for o in out]


def _ms(t, name, on):
    ms = getattr(t, name + "_kernel_ms")(on)
    return (ms,) if N_MS[name] == 1 else tuple(ms)


def test_the_match_batch_has_matched_and_unmatched_jobs():
    """(CPU) the two searches are the smallest generated ones with this property in either mode"""
    for mode in mc.BOTH:
        for s in _inputs("match")[mode]:
            st = mo.sequential(s, match_params(mode, 1)).status
            assert (st == MATCH_OK).any() and (st != MATCH_OK).any()


@pytest.mark.gpu
def test_each_bracket_alone_times_its_call_and_moves_no_bit():
    t = Tracker(track_config())
    try:
        for name in CALLS:
            assert _ms(t, name, False) == (-1.0,) * N_MS[name]
        base = {name: _run(t, name) for name in CALLS}
        for name in CALLS:                                       # an untimed call leaves -1
            assert _ms(t, name, False) == (-1.0,) * N_MS[name]
        for name in CALLS:
            before = {m: _ms(t, m, False) for m in CALLS}
            _ms(t, name, True)
            outs = {m: _run(t, m) for m in CALLS}
            after = {m: _ms(t, m, m == name) for m in CALLS}
            for m in CALLS:
                assert outs[m] == base[m], (name, m)
                if m != name:
                    assert after[m] == before[m], (name, m)
            assert after[name] != before[name]
            assert all(math.isfinite(v) and v >= 0 for v in after[name]), after[name]
            print(name, after[name])
            assert _ms(t, name, False) == after[name]            # switched off: the value stays ...
            assert _run(t, name) == base[name]
            assert _ms(t, name, False) == after[name]            # ... through a further call
    finally:
        t.close()
