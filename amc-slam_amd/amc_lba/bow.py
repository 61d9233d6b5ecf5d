"""ORBmatcher::SearchByBoW through the C ABI (lba_match_bow on an lba_tracker): a batch of pairs, one GPU wave per
(pair, vocabulary node both sides hold).  Both overloads: BOW_KF is (pKF1, pKF2, vpMatches12) of
LoopClosing::DetectCommonRegionsFromBoW (src/ORBmatcher.cc:805-945), BOW_FRAME is (pKF, F, vpMapPointMatches) of
Tracking::TrackReferenceKeyFrame (:227-421).  The keyframe arrays are those of lba_match_epipolar
(amc_lba.epipolar: `epi_feats`, `feat_vec_csr`, `pack_epi_keyframes`); a frame is one more entry of them.

`Tracker.match_bow` is the call.  The caller's side on plain arrays: `bow_pairs` (one side 1 against many side 2),
`bow_matches` (vpMatches12 as index pairs), `frame_matches` (the frame overload's scatter), `bow_merge`
(LoopClosing.cc:499-516, whose result feeds sim3_ransac.sim3_ransac_rows).  `make_bow_pairs` makes synthetic pairs.
"""
import ctypes

import numpy as np

from . import LbaError
from .abi import BOW_PAIR_DTYPE, BOW_ROW_DTYPE, EPI_FEAT_DTYPE, EPI_KF_DTYPE, ptr
from .epipolar import pack_epi_keyframes
from .match import _bind as _bind_match, tracker_last_error
from .track import kernel_ms

BOW_KF, BOW_FRAME = 0, 1
BOW_OK, BOW_NO_POINT, BOW_NO_NODE, BOW_NO_CAND, BOW_RATIO, BOW_ROT = range(6)
BOW_STATUS_NAMES = ("OK", "NO_POINT", "NO_NODE", "NO_CAND", "RATIO", "ROT")
BOW_MAX_NODE = 2048     # LBA_E_LIMIT above: entries of one node's list on side 2
BOW_LDS_CAP = 512       # candidates of a node the kernel stages in LDS; the ones behind are read from global memory
TH_LOW = 50


class LbaBowParams(ctypes.Structure):
    """lba_bow_params: the overload, TH_LOW, mfNNratio, mbCheckOrientation."""
    _fields_ = [("mode", ctypes.c_int32), ("th_low", ctypes.c_int32), ("nn_ratio", ctypes.c_float),
                ("check_orientation", ctypes.c_int32)]


def bow_params(mode=BOW_KF, th_low=TH_LOW, nn_ratio=0.9, check_orientation=True):
    """The defaults are LoopClosing's matcherBoW(0.9, true); TrackReferenceKeyFrame builds ORBmatcher(0.7, true)."""
    return LbaBowParams(int(mode), int(th_low), float(nn_ratio), int(bool(check_orientation)))


def _bind():
    L = _bind_match()
    if not getattr(L, "_bow_bound", False):
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.lba_match_bow.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp, i32, ctypes.POINTER(LbaBowParams)]
        L._bow_bound = True
    return L


def match_bow(tracker, pairs, ekfs, feats, node_id, node_start, node_feat, params=None, out=None):
    """Every keypoint of side 1 of every pair.  `pairs` (BOW_PAIR_DTYPE) is modified in place when it has the right
    dtype and layout (n_matches), copied otherwise.  `params`: an LbaBowParams (bow_params(...)) or None for
    BOW_KF, 50, 0.9, 1.  Returns (pairs, out): out [max(out0 + n_feat(kf1))] BOW_ROW_DTYPE, a pair's rows at its out0
    (`out`: the caller's array of at least that length, written in place)."""
    pairs = np.ascontiguousarray(pairs, BOW_PAIR_DTYPE)
    ekfs = np.ascontiguousarray(ekfs, EPI_KF_DTYPE)
    feats = np.ascontiguousarray(feats, EPI_FEAT_DTYPE)
    node_id, node_start, node_feat = (np.ascontiguousarray(a, np.int32) for a in (node_id, node_start, node_feat))
    ok = (pairs["kf1"] >= 0) & (pairs["kf1"] < len(ekfs))
    n_out = int((pairs["out0"][ok] + ekfs["n_feat"][pairs["kf1"][ok]]).max()) if ok.any() else 0
    if out is None:
        out = np.zeros(max(n_out, 0), BOW_ROW_DTYPE)
    assert out.dtype == BOW_ROW_DTYPE and out.flags["C_CONTIGUOUS"] and len(out) >= n_out
    rc = _bind().lba_match_bow(tracker.h, ptr(pairs), len(pairs), ptr(out), len(out), ptr(ekfs), len(ekfs), ptr(feats),
                               len(feats), ptr(node_id), ptr(node_start), len(node_id), ptr(node_feat), len(node_feat),
                               ctypes.byref(params) if params is not None else None)
    if rc != 0:
        raise LbaError(rc, "lba_match_bow failed: " + tracker_last_error(tracker))
    return pairs, out


def match_bow_kernel_ms(tracker, on=True):
    """track.kernel_ms for lba_match_bow's launch (k_bow_match)"""
    return kernel_ms(tracker, "lba_match_bow_profile", on)


def bow_pairs(kf1, kf2s, ekfs):
    """lba_bow_pair records of one side 1 (`kf1`: an index, or one per pair) against the keyframes `kf2s`, their out
    ranges one behind the other: DetectCommonRegionsFromBoW's loop over a candidate's covisible keyframes, with
    mpCurrentKF as kf1"""
    kf2s = np.atleast_1d(np.asarray(kf2s, np.int64))
    kf1 = np.broadcast_to(np.asarray(kf1, np.int64), kf2s.shape)
    pairs = np.zeros(len(kf2s), BOW_PAIR_DTYPE)
    pairs["kf1"], pairs["kf2"] = kf1, kf2s
    n1 = np.asarray(ekfs["n_feat"], np.int64)[kf1]
    pairs["out0"] = np.concatenate([[0], np.cumsum(n1)[:-1]]) if len(kf2s) else 0
    return pairs


def bow_rows(pair, out, ekfs):
    """a pair's rows of `out`"""
    return out[int(pair["out0"]):int(pair["out0"]) + int(ekfs[int(pair["kf1"])]["n_feat"])]


def bow_matches(pair, out, ekfs=None):
    """vpMatches12 of one pair as [n, 2] (idx1, idx2) in ascending idx1: the keypoints of side 1 whose entry is not
    NULL and the keypoint of side 2 whose point it holds.  `out`: the call's, with `ekfs`; or the pair's own rows."""
    rows = out if ekfs is None else bow_rows(pair, out, ekfs)
    idx1 = np.flatnonzero(rows["status"] == BOW_OK)
    return np.stack([idx1, rows["idx2"][idx1].astype(np.int64)], axis=1).reshape(-1, 2)


def frame_matches(pair, out, n_feat2, ekfs=None):
    """The frame overload's vpMapPointMatches as keypoint indices: [n_feat2] int64, entry idx2 = the keypoint idx1 of
    the keyframe whose point the frame's keypoint idx2 gets (vpMapPointMatches[row.idx2] = point of idx1), -1 where
    NULL.  idx2 is unique among a pair's accepted rows, so the scatter has no collisions."""
    m = bow_matches(pair, out, ekfs)
    res = np.full(int(n_feat2), -1, np.int64)
    res[m[:, 1]] = m[:, 0]
    return res


def bow_merge(rows_per_pair, point_id2_per_pair, bad=()):
    """LoopClosing.cc:499-516 on plain arrays.  rows_per_pair[j]: the BOW_ROW_DTYPE rows of (mpCurrentKF, vpCovKFi[j]),
    or None where the reference skipped the keyframe (:487); point_id2_per_pair[j] [n_feat(kf2 j)]: the id of the map
    point of each of its keypoints, -1 for none; `bad`: the ids of the points that are bad by now.  In the order of
    the pairs, then of k: a match whose point is new to spMatchedMPi sets vpMatchedPoints[k] and vpKeyFrameMatchedMP[k]
    (a later pair may overwrite an entry with another new point, as the reference does).
    Returns (point [n1] int64, the id in vpMatchedPoints[k] or -1; pair [n1] int64, the j of vpKeyFrameMatchedMP[k] or
    -1; numBoWMatches).  `point >= 0` is the `match` of sim3_ransac.sim3_ransac_rows."""
    bad = set(int(b) for b in bad)
    n1 = max((len(r) for r in rows_per_pair if r is not None), default=0)
    point, pair = np.full(n1, -1, np.int64), np.full(n1, -1, np.int64)
    seen, n = set(), 0
    for j, rows in enumerate(rows_per_pair):
        if rows is None:
            continue
        ids = np.asarray(point_id2_per_pair[j], np.int64)
        for k in np.flatnonzero(rows["status"] == BOW_OK):
            mp = int(ids[rows["idx2"][k]])
            if mp < 0 or mp in bad or mp in seen:
                continue
            seen.add(mp)
            n += 1
            point[k], pair[k] = mp, j
    return point, pair, n


def flip_many(desc, n_bits, rng):
    """match.flip_bits on every row: desc [n, 8] uint32 with n_bits[i] distinct random bits of row i flipped"""
    desc = np.asarray(desc, np.uint32).reshape(-1, 8)
    n_bits = np.broadcast_to(np.asarray(n_bits, np.int64), (len(desc),))
    rank = rng.random((len(desc), 256)).argsort(axis=1).argsort(axis=1)
    mask = np.packbits(rank < n_bits[:, None], axis=1, bitorder="little").view("<u4").reshape(-1, 8)
    return desc ^ mask


def make_bow_pairs(n_pairs=1, n_feat=300, n_nodes=20, seed=0, cluster=3, cluster_bits=(4, 24), bits=(0, 14),
                   seen_frac=0.6, clutter_frac=0.25, has_point_frac=0.85, no_node_frac=0.03, rot_outlier_frac=0.15,
                   shared_frac=0.5):
    """Synthetic SearchByBoW inputs: a current keyframe (index 0) and `n_pairs` others, `n_feat` keypoints each, with
    the descriptor conventions of epipolar.make_epi_pairs (a random 256-bit base, match.flip_bits noise, the vocabulary
    node from the BASE: base[0] % n_nodes).  The current keyframe's keypoints come in clusters of `cluster` members: a
    member is the cluster's base with some of `cluster_bits` flipped, all in the base's node, so the members are each
    other's second best and compete for the same keypoints of the other side.  Another keyframe sees a share
    `seen_frac` of the members (the member's descriptor with some of `bits` flipped, the member's angle turned by the
    pair's rotation, or by anything for a share `rot_outlier_frac`); a share `clutter_frac` of its other keypoints
    takes a random cluster's base and node with `cluster_bits` flipped, the rest is random.  Keypoints are in random
    order.  A share `has_point_frac` of all keypoints has a map point; a share `no_node_frac` is in no node.  The
    point of a seen member is the member's own id in a share `shared_frac` of the cases (so the same point turns up in
    several keyframes, for bow_merge), a fresh id otherwise.
    Returns (pairs, ekfs, feats, node_id, node_start, node_feat, truth) with truth = {"nodes": node per keypoint per
    keyframe, "point_id": per keyframe the point id per keypoint or -1, "member": per other keyframe the keypoint of
    the current one that it shows or -1}."""
    rng = np.random.default_rng([seed, 0xB0])
    n_cl = max(1, n_feat // cluster)

    def rand_desc(n):
        return rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)

    def nbits(lo_hi, n):
        return rng.integers(lo_hi[0], lo_hi[1] + 1, n)

    def feats_of(desc, angle, has):
        f = np.zeros(len(desc), EPI_FEAT_DTYPE)
        f["desc"], f["angle"], f["has_point"] = desc, angle, has
        f["u_right"], f["scale"], f["sigma2"] = -1.0, 1.0, 1.0
        return f

    base = rand_desc(n_cl)
    cl_node = base[:, 0].astype(np.int64) % n_nodes
    cl = rng.integers(0, n_cl, n_feat) if n_feat else np.zeros(0, np.int64)
    cl[:min(n_feat, n_cl * cluster)] = np.repeat(np.arange(n_cl), cluster)[:n_feat]
    cl = rng.permutation(cl)
    desc0 = flip_many(base[cl], nbits(cluster_bits, n_feat), rng)
    ang0 = rng.uniform(0, 360, n_feat).astype(np.float32)
    node0 = np.where(rng.random(n_feat) < no_node_frac, -1, cl_node[cl])
    has0 = rng.random(n_feat) < has_point_frac
    all_f, all_nodes = [feats_of(desc0, ang0, has0)], [node0]
    point_id = [np.where(has0, np.arange(n_feat), -1)]
    members, next_id = [], n_feat
    for p in range(n_pairs):
        turn = rng.uniform(0, 360)
        src = np.where(rng.random(n_feat) < seen_frac, rng.permutation(n_feat), -1)     # a member at most once
        near = (src < 0) & (rng.random(n_feat) < clutter_frac)
        c2 = rng.integers(0, n_cl, n_feat)
        d = rand_desc(n_feat)
        node = d[:, 0].astype(np.int64) % n_nodes
        ang = rng.uniform(0, 360, n_feat)
        s = src >= 0
        d[s] = flip_many(desc0[src[s]], nbits(bits, int(s.sum())), rng)
        node[s] = cl_node[cl[src[s]]]
        off = np.where(rng.random(int(s.sum())) < rot_outlier_frac, rng.uniform(0, 360, int(s.sum())), turn + rng.normal(0, 4.0, int(s.sum())))
        ang[s] = (ang0[src[s]].astype(np.float64) - off) % 360.0
        d[near] = flip_many(base[c2[near]], nbits(cluster_bits, int(near.sum())), rng)
        node[near] = cl_node[c2[near]]
        node = np.where(rng.random(n_feat) < no_node_frac, -1, node)
        has = rng.random(n_feat) < has_point_frac
        ids = next_id + np.arange(n_feat)
        next_id += n_feat
        share = s & (rng.random(n_feat) < shared_frac)
        ids[share] = src[share]
        all_f.append(feats_of(d, ang.astype(np.float32), has))
        all_nodes.append(node)
        point_id.append(np.where(has, ids, -1))
        members.append(src)
    ekfs, feats, node_id, node_start, node_feat = pack_epi_keyframes(all_f, all_nodes)
    pairs = bow_pairs(0, 1 + np.arange(n_pairs), ekfs)
    return pairs, ekfs, feats, node_id, node_start, node_feat, {"nodes": all_nodes, "point_id": point_id, "member": members}
