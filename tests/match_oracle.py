"""numpy restatement of ORBmatcher's two projection searches (src/ORBmatcher.cc:43-217, :1439-1568, with
MultiFrame::GetFeaturesInArea, src/Frame.cc:608-673, and ComputeThreeMaxima, :1697-1738) on the arrays
lba_match_project takes: np.float32 scalars for every gate, Python ints for the rest.

`sequential` is the reference's loop, job after job.  `by_rounds` is a second, independent resolve: the rounds of
k_match_resolve per camera, which must give the same outputs and defines `rounds`.  `alone` runs
every job by itself against the entry `taken` state (what a matcher without the resolve phase would give).
"""
import numpy as np

from amc_lba.match import (GRID_CELLS, GRID_COLS, GRID_ROWS, HISTO_LENGTH, MATCH_BEST, MATCH_NO_CAND, MATCH_OK,
                           MATCH_RATIO, MATCH_RATIO_FAIL, MATCH_ROT, MATCH_TOO_FAR)

F = np.float32
INT_LO, INT_HI = F(-2147483648.0), F(2147483648.0)


class Result:
    def __init__(self, n_jobs, n_feat, n_cam):
        self.feat = np.full(n_jobs, -1, np.int32)
        self.status = np.full(n_jobs, -1, np.int32)
        self.best_dist = np.full(n_jobs, 256, np.int32)
        self.best_dist2 = np.full(n_jobs, 256, np.int32)
        self.job = np.full(n_feat, -1, np.int32)
        self.rounds = np.zeros(n_cam, np.int32)
        self.n_matches = self.n_matches_mono = 0

    def same_outputs(self, o):
        return all((getattr(self, k) == getattr(o, k)).all() for k in ("feat", "status", "best_dist", "best_dist2", "job")) \
            and self.n_matches == o.n_matches and self.n_matches_mono == o.n_matches_mono


def _cell(v, n):
    """(int)v for a float32 floor / ceil value within int's range, clamped to [-1, n] first; None otherwise (quirk e)"""
    if not (v >= INT_LO and v < INT_HI):
        return None
    return int(min(max(v, F(-1.0)), F(n)))


def cell_rect(x, y, r, cam):
    """nMinCellX, nMaxCellX, nMinCellY, nMaxCellY of GetFeaturesInArea, or None where it returns nothing"""
    x, y, r = F(x), F(y), F(r)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(r)):
        return None
    mx, my, wi, hi = F(cam["min_x"]), F(cam["min_y"]), F(cam["grid_w_inv"]), F(cam["grid_h_inv"])
    with np.errstate(all="ignore"):
        x0 = _cell(np.floor((x - mx - r) * wi), GRID_COLS)
        x1 = _cell(np.ceil((x - mx + r) * wi), GRID_COLS)
        y0 = _cell(np.floor((y - my - r) * hi), GRID_ROWS)
        y1 = _cell(np.ceil((y - my + r) * hi), GRID_ROWS)
    if None in (x0, x1, y0, y1):
        return None
    x0 = max(0, x0)
    if x0 >= GRID_COLS:
        return None
    x1 = min(GRID_COLS - 1, x1)
    if x1 < 0:
        return None
    y0 = max(0, y0)
    if y0 >= GRID_ROWS:
        return None
    y1 = min(GRID_ROWS - 1, y1)
    if y1 < 0:
        return None
    return x0, x1, y0, y1


def capacity(s, k):
    """the features in job k's cell rectangle, before any gate"""
    j = s.jobs[k]
    R = cell_rect(j["x"], j["y"], j["radius"], s.cams[j["cam"]])
    if R is None:
        return 0
    cs = s.cell_start[int(j["cam"]) * GRID_CELLS:]
    return sum(max(0, int(cs[ix * GRID_ROWS + R[3] + 1]) - int(cs[ix * GRID_ROWS + R[2]])) for ix in range(R[0], R[1] + 1))


def _ints(desc):
    return [int.from_bytes(np.ascontiguousarray(d).tobytes(), "little") for d in desc]


def candidates(s, prm):
    """per job the list of (feature, distance, octave) GetFeaturesInArea and the stereo gate leave, in order"""
    fd, jd = _ints(s.feats["desc"]), _ints(s.jobs["desc"])
    fx, fy, fo, fu = (s.feats[k] for k in ("x", "y", "octave", "u_right"))
    out = []
    for k, j in enumerate(s.jobs):
        lst = []
        out.append(lst)
        x, y, r, c = F(j["x"]), F(j["y"]), F(j["radius"]), int(j["cam"])
        R = cell_rect(x, y, r, s.cams[c])
        if R is None:
            continue
        lo, hi = int(j["min_level"]), int(j["max_level"])
        check = lo > 0 or hi >= 0
        for ix in range(R[0], R[1] + 1):
            for iy in range(R[2], R[3] + 1):
                cell = c * GRID_CELLS + ix * GRID_ROWS + iy
                for f in s.cell_feat[s.cell_start[cell]:s.cell_start[cell + 1]]:
                    f = int(f)
                    if check:
                        if fo[f] < lo:
                            continue
                        if hi >= 0 and fo[f] > hi:
                            continue
                    if not (abs(F(fx[f]) - x) < r and abs(F(fy[f]) - y) < r):
                        continue
                    if c == prm.stereo_cam:
                        u = F(np.trunc(fu[f])) if prm.ur_truncate else F(fu[f])
                        if u > 0 and abs(F(j["ur"]) - u) > r:
                            continue
                    lst.append((f, bin(fd[f] ^ jd[k]).count("1"), int(fo[f])))
    return out


def _scan(lst, taken, mode):
    """the loop over vIndices: (bestDist, bestLevel, bestDist2, bestLevel2, bestIdx, candidates looked at)"""
    best, lvl, best2, lvl2, idx, n = 256, -1, 256, -1, -1, 0
    for f, d, o in lst:
        if taken[f]:
            continue
        n += 1
        if mode == MATCH_RATIO:
            if d < best:
                best2, best, lvl2, lvl, idx = best, d, lvl, o, f
            elif d < best2:
                lvl2, best2 = o, d
        elif d < best:
            best, idx = d, f
    return best, lvl, best2, lvl2, idx, n


def _decide(scan, prm):
    best, lvl, best2, lvl2, idx, n = scan
    if n == 0:
        return MATCH_NO_CAND
    if not best <= prm.th_high:
        return MATCH_TOO_FAR
    if prm.mode == MATCH_RATIO and lvl == lvl2 and F(best) > F(prm.nn_ratio) * F(best2):
        return MATCH_RATIO_FAIL
    return MATCH_OK


def rot_bin(a_last, a_cur):
    rot = F(a_last) - F(a_cur)
    if rot < 0:
        rot = rot + F(360.0)
    v = rot * (F(1.0) / F(HISTO_LENGTH))
    b = int(np.sign(v) * np.floor(abs(v) + F(0.5)))
    return 0 if b == HISTO_LENGTH or not 0 <= b < HISTO_LENGTH else b


def three_maxima(sizes):
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, n in enumerate(sizes):
        if n > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, n, i2, i1, i
        elif n > max2:
            max3, max2, i3, i2 = max2, n, i2, i
        elif n > max3:
            max3, i3 = n, i
    if F(max2) < F(0.1) * F(max1):
        i2 = i3 = -1
    elif F(max3) < F(0.1) * F(max1):
        i3 = -1
    return i1, i2, i3


def _finish(s, prm, res):
    ok = np.flatnonzero(res.status == MATCH_OK)
    res.n_matches = len(ok)
    res.n_matches_mono = int((s.jobs["cam"][ok] < s.n_cam - 1).sum())
    if prm.mode == MATCH_BEST and prm.check_orientation:
        bins = [rot_bin(s.jobs["angle"][k], s.feats["angle"][res.feat[k]]) for k in ok]
        keep = three_maxima(np.bincount(np.array(bins, np.int64), minlength=HISTO_LENGTH))
        for k, b in zip(ok, bins):
            if b not in keep:
                res.status[k] = MATCH_ROT
                res.job[res.feat[k]] = -1
                res.n_matches -= 1
    return res


def _record(res, k, scan, st):
    res.status[k], res.best_dist[k], res.best_dist2[k] = st, scan[0], scan[2]
    res.feat[k] = scan[4] if st == MATCH_OK else -1


def sequential(s, prm, cands=None):
    cands = candidates(s, prm) if cands is None else cands
    res = Result(len(s.jobs), len(s.feats), s.n_cam)
    taken = [bool(t) for t in s.feats["taken"]]
    for k, lst in enumerate(cands):
        scan = _scan(lst, taken, prm.mode)
        st = _decide(scan, prm)
        _record(res, k, scan, st)
        if st == MATCH_OK:
            res.job[scan[4]] = k
            if s.jobs["blocks"][k]:
                taken[scan[4]] = True
    return _finish(s, prm, res)


def alone(s, prm, cands=None):
    """every job by itself against the entry `taken` state: (status, feat)"""
    cands = candidates(s, prm) if cands is None else cands
    taken = [bool(t) for t in s.feats["taken"]]
    status, feat = np.zeros(len(cands), np.int32), np.full(len(cands), -1, np.int32)
    for k, lst in enumerate(cands):
        scan = _scan(lst, taken, prm.mode)
        status[k] = _decide(scan, prm)
        if status[k] == MATCH_OK:
            feat[k] = scan[4]
    return status, feat


def by_rounds(s, prm, cands=None):
    """the rounds of k_match_resolve, camera by camera: in a round every pending job puts its index on each of its
    untaken candidates, the smallest index staying; a job that finds its own index on all of them is final"""
    cands = candidates(s, prm) if cands is None else cands
    res = Result(len(s.jobs), len(s.feats), s.n_cam)
    for c in range(s.n_cam):
        pending = [k for k in range(len(s.jobs)) if s.jobs["cam"][k] == c]
        taken = {f for f in range(len(s.feats)) if s.feats["taken"][f]}
        while pending:
            res.rounds[c] += 1
            owner = {}
            for k in pending:
                for f, _, _ in cands[k]:
                    if f not in taken:
                        owner[f] = min(owner.get(f, k), k)
            final = [k for k in pending if all(owner[f] == k for f, _, _ in cands[k] if f not in taken)]
            now = [f in taken for f in range(len(s.feats))]      # the round's start: what every final job sees
            for k in final:
                scan = _scan(cands[k], now, prm.mode)
                st = _decide(scan, prm)
                _record(res, k, scan, st)
                if st == MATCH_OK:
                    res.job[scan[4]] = k
                    if s.jobs["blocks"][k]:
                        taken.add(scan[4])
            done = set(final)
            pending = [k for k in pending if k not in done]
    return _finish(s, prm, res)
