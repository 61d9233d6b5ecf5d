"""Two independent numpy restatements of ORBmatcher::SearchByBoW, both overloads (src/ORBmatcher.cc:805-945 and
:227-421), for one pair on the arrays of lba_match_bow:

  sequential   the merge walk and the two loops as written, the matched flag carried from keypoint to keypoint;
  by_node      per common node the full distance matrix first, then per idx1 in list order a masked two-smallest
               with the first-position arg-min.  No state outside the node.

Their agreement (tests/test_bow_cases.py) is what licenses the kernel's form: one wave per node, the candidates in
parallel.  `sequential` also takes the variants a wrong device would compute, used only to show that the cases bite:
flag=False (never mark matched), tie="last", ratio_double (the product of the ratio test in double)."""
from collections import namedtuple

import numpy as np

from epi_oracle import HISTO, rot_bin, three_maxima

KF, FRAME = 0, 1
OK, NO_POINT, NO_NODE, NO_CAND, RATIO, ROT = range(6)
_POP = np.array([bin(i).count("1") for i in range(65536)], np.int64)

Job = namedtuple("Job", "f1 f2 fv1 fv2 prm")          # fv: (node_id, node_start, node_feat) of a side
Result = namedtuple("Result", "idx2 dist dist2 status n_matches")
PRM = dict(mode=KF, th_low=50, nn_ratio=0.9, check_orientation=1)


def jobs_of(c, prm=None):
    """the pairs of a case (tests/bow_cases.py: the arrays of the call) as Jobs"""
    out = []
    for P in c.pairs:
        side = []
        for k in (int(P["kf1"]), int(P["kf2"])):
            E = c.ekfs[k]
            ids = c.node_id[E["node0"]:E["node0"] + E["n_node"]]
            st = c.node_start[E["node0"]:E["node0"] + E["n_node"] + 1] if E["n_node"] else np.zeros(1, np.int32)
            nf = c.node_feat[E["nf0"]:E["nf0"] + st[-1]]
            side.append((c.feats[E["feat0"]:E["feat0"] + E["n_feat"]], (ids, st, nf)))
        out.append(Job(side[0][0], side[1][0], side[0][1], side[1][1], dict(PRM, **(c.prm if prm is None else prm))))
    return out


def hamming(d1, d2):
    """the 256-bit distance of d1 [8] to every row of d2 [n, 8]"""
    x = np.bitwise_xor(np.asarray(d2, np.uint32), np.asarray(d1, np.uint32)[None, :])
    return (_POP[x & 0xFFFF] + _POP[x >> 16]).sum(axis=1)


def hamming_matrix(d1, d2):
    """[n1, n2] by unpacked bits (not the table of `hamming`)"""
    b1 = np.unpackbits(np.ascontiguousarray(d1, "<u4").view(np.uint8).reshape(len(d1), 32), axis=1).astype(np.int64)
    b2 = np.unpackbits(np.ascontiguousarray(d2, "<u4").view(np.uint8).reshape(len(d2), 32), axis=1).astype(np.int64)
    return b1 @ (1 - b2).T + (1 - b1) @ b2.T


def accept(b1, b2, prm, ratio_double=False):
    """the status after the inner loop: the threshold (`<` or `<=` by overload), then the float ratio test"""
    if not (b1 <= prm["th_low"] if prm["mode"] == FRAME else b1 < prm["th_low"]):
        return NO_CAND
    r = np.float32(prm["nn_ratio"])
    if ratio_double:
        return OK if float(b1) < float(r) * float(b2) else RATIO
    return OK if np.float32(b1) < np.float32(r * np.float32(b2)) else RATIO


def _finish(job, idx2, dist, dist2, status):
    """nmatches and the rotation pass (:924-942, :400-418): the bins that are NOT one of the three maxima lose their
    matches"""
    n = int((status == OK).sum())
    if job.prm["check_orientation"]:
        ok = np.flatnonzero(status == OK)
        bins = np.array([rot_bin(job.f1["angle"][i], job.f2["angle"][idx2[i]]) for i in ok], np.int64)
        maxima = three_maxima(np.bincount(bins, minlength=HISTO)) if len(ok) else (-1, -1, -1)
        for i, b in zip(ok, bins):
            if b not in maxima:
                status[i] = ROT
                n -= 1
    return Result(idx2, dist, dist2, status, n)


def _blank(n1):
    return np.full(n1, -1, np.int64), np.full(n1, 256, np.int64), np.full(n1, 256, np.int64), np.full(n1, NO_NODE, np.int64)


def _lower_bound(ids, lo, key):
    return lo + int(np.searchsorted(ids[lo:], key, side="left"))


def sequential(job, flag=True, tie="first", ratio_double=False):
    """The function as written."""
    p = job.prm
    idx2_out, dist_out, dist2_out, status = _blank(len(job.f1))
    matched2 = np.zeros(len(job.f2), bool)
    (id1, s1, nf1), (id2, s2, nf2) = job.fv1, job.fv2
    a = b = 0
    while a < len(id1) and b < len(id2):
        if id1[a] == id2[b]:
            l2 = nf2[s2[b]:s2[b + 1]]
            for idx1 in nf1[s1[a]:s1[a + 1]]:
                if not job.f1["has_point"][idx1]:
                    status[idx1] = NO_POINT
                    continue
                best1, best_idx2, best2 = 256, -1, 256
                d = hamming(job.f1["desc"][idx1], job.f2["desc"][l2]) if len(l2) else []
                for k, i2 in enumerate(l2):
                    if matched2[i2]:
                        continue
                    if p["mode"] == KF and not job.f2["has_point"][i2]:
                        continue
                    dist = int(d[k])
                    if dist < best1 or (tie == "last" and dist == best1 and dist < 256):
                        best2, best1, best_idx2 = best1, dist, int(i2)
                    elif dist < best2:
                        best2 = dist
                st = accept(best1, best2, p, ratio_double)
                if st == OK and flag:
                    matched2[best_idx2] = True
                idx2_out[idx1], dist_out[idx1], dist2_out[idx1], status[idx1] = best_idx2, best1, best2, st
            a += 1
            b += 1
        elif id1[a] < id2[b]:
            a = _lower_bound(id1, a, id2[b])
        else:
            b = _lower_bound(id2, b, id1[a])
    return _finish(job, idx2_out, dist_out, dist2_out, status)


def by_node(job):
    p = job.prm
    idx2_out, dist_out, dist2_out, status = _blank(len(job.f1))
    (id1, s1, nf1), (id2, s2, nf2) = job.fv1, job.fv2
    pos2 = {int(n): k for k, n in enumerate(id2)}
    for a, node in enumerate(id1):
        b = pos2.get(int(node))
        if b is None:
            continue
        l1, l2 = nf1[s1[a]:s1[a + 1]], nf2[s2[b]:s2[b + 1]]
        D = hamming_matrix(job.f1["desc"][l1], job.f2["desc"][l2])
        free = np.ones(len(l2), bool) if p["mode"] == FRAME else job.f2["has_point"][l2] != 0
        for r, idx1 in enumerate(l1):
            if not job.f1["has_point"][idx1]:
                status[idx1] = NO_POINT
                continue
            d = np.where(free, D[r], 256)
            two = np.sort(np.concatenate([d, [256, 256]]))[:2]
            first = int(np.argmin(d)) if len(d) and two[0] < 256 else -1       # argmin: the first position of the minimum
            st = accept(int(two[0]), int(two[1]), p)
            if st == OK:
                free[first] = False
            idx2_out[idx1], dist_out[idx1], dist2_out[idx1], status[idx1] = (l2[first] if first >= 0 else -1), two[0], two[1], st
    return _finish(job, idx2_out, dist_out, dist2_out, status)


def same(a, b):
    return all((getattr(a, f) == getattr(b, f)).all() for f in ("idx2", "dist", "dist2", "status")) and a.n_matches == b.n_matches


def rows_differing(a, b):
    """the number of side-1 keypoints on which two Results differ in any field"""
    diff = np.zeros(len(a.status), bool)
    for f in ("idx2", "dist", "dist2", "status"):
        diff |= getattr(a, f) != getattr(b, f)
    return int(diff.sum())
