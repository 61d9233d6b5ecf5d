"""ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:947-1131) through the C ABI (lba_match_epipolar on an
lba_tracker): a batch of (keyframe, neighbour) pairs, one GPU lane per keypoint of KF1.  Its matches are the rows of
lba_triangulate (amc_lba.triangulate), with which it shares the keyframe and camera records.

`Tracker.match_epipolar` is the call.  The caller's side on plain arrays: `feat_vec_csr` (mFeatVec as three arrays),
`epi_feats` (the feature records from the per-keyframe mapping `tri_rows` takes), `pack_epi_keyframes` (several
keyframes one behind the other) and `epi_matches` (vMatchedPairs).  `make_epi_pairs` makes synthetic pairs.
"""
import ctypes

import numpy as np

from . import LbaError
from .abi import (EPI_FEAT_DTYPE, EPI_KF_DTYPE, EPI_PAIR_DTYPE, EPI_ROW_DTYPE, TRI_CAM_DTYPE, TRI_KF_DTYPE, ptr)
from .match import _bind as _bind_match, flip_bits, tracker_last_error
from .track import kernel_ms
from .triangulate import TRI_K, scale_pyramid, tri_keyframes

EPI_OK, EPI_HAS_POINT, EPI_NOT_STEREO, EPI_NO_NODE, EPI_NO_MATCH, EPI_ROT = range(6)
EPI_STATUS_NAMES = ("OK", "HAS_POINT", "NOT_STEREO", "NO_NODE", "NO_MATCH", "ROT")
EPI_MAX_CAM = 64       # LBA_E_LIMIT above, as lba_triangulate
TH_LOW = 50


class LbaEpiParams(ctypes.Structure):
    """lba_epi_params: TH_LOW, bOnlyStereo, bCoarse, mbCheckOrientation."""
    _fields_ = [("th_low", ctypes.c_int32), ("only_stereo", ctypes.c_int32), ("coarse", ctypes.c_int32),
                ("check_orientation", ctypes.c_int32)]


def epi_params(th_low=TH_LOW, only_stereo=False, coarse=False, check_orientation=False):
    """CreateNewMapPoints calls SearchForTriangulation(kf1, kf2, matches, false, false) on ORBmatcher(0.6f, false)."""
    return LbaEpiParams(int(th_low), int(bool(only_stereo)), int(bool(coarse)), int(bool(check_orientation)))


def _bind():
    L = _bind_match()
    if not getattr(L, "_epi_bound", False):
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.lba_match_epipolar.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, vp, i32, vp, vp, i32, vp, i32,
                                         ctypes.POINTER(LbaEpiParams)]
        L._epi_bound = True
    return L


def match_epipolar(tracker, pairs, kfs, ekfs, cams, n_cam, feats, node_id, node_start, node_feat, params=None, out=None):
    """Every keypoint of KF1 of every pair.  `pairs` (EPI_PAIR_DTYPE) is modified in place when it has the right dtype
    and layout (n_matches), copied otherwise.  `params`: an LbaEpiParams (epi_params(...)) or None for 50, 0, 0, 0.
    Returns (pairs, out): out [max(out0 + n_feat(kf1))] EPI_ROW_DTYPE, a pair's rows at its out0 (`out`: the caller's
    array of at least that length, written in place)."""
    pairs = np.ascontiguousarray(pairs, EPI_PAIR_DTYPE)
    kfs = np.ascontiguousarray(kfs, TRI_KF_DTYPE)
    ekfs = np.ascontiguousarray(ekfs, EPI_KF_DTYPE)
    cams = np.ascontiguousarray(cams, TRI_CAM_DTYPE)
    feats = np.ascontiguousarray(feats, EPI_FEAT_DTYPE)
    node_id, node_start, node_feat = (np.ascontiguousarray(a, np.int32) for a in (node_id, node_start, node_feat))
    ok = (pairs["kf1"] >= 0) & (pairs["kf1"] < len(ekfs))
    n_out = int((pairs["out0"][ok] + ekfs["n_feat"][pairs["kf1"][ok]]).max()) if ok.any() else 0
    if out is None:
        out = np.zeros(max(n_out, 0), EPI_ROW_DTYPE)
    assert out.dtype == EPI_ROW_DTYPE and out.flags["C_CONTIGUOUS"] and len(out) >= n_out
    rc = _bind().lba_match_epipolar(tracker.h, ptr(pairs), len(pairs), ptr(out), len(out), ptr(kfs), ptr(ekfs), len(kfs),
                                    ptr(cams), len(cams), int(n_cam), ptr(feats), len(feats), ptr(node_id),
                                    ptr(node_start), len(node_id), ptr(node_feat), len(node_feat),
                                    ctypes.byref(params) if params is not None else None)
    if rc != 0:
        raise LbaError(rc, "lba_match_epipolar failed: " + tracker_last_error(tracker))
    return pairs, out


def match_epipolar_kernel_ms(tracker, on=True):
    """track.kernel_ms for lba_match_epipolar's two launches: (k_epi_tables, k_epi_match)"""
    return kernel_ms(tracker, "lba_match_epipolar_profile", on, 2)


def feat_vec_csr(nodes_per_keypoint):
    """A keyframe's mFeatVec from one node id per keypoint (-1: in no node): (node_id [n_node] strictly ascending,
    node_start [n_node + 1] from 0, node_feat), the keypoints of a node in ascending order, as
    DBoW2::FeatureVector::addFeature leaves them when ComputeBoW walks the descriptors in order (KeyFrame.cc:103-110)."""
    nodes = np.asarray(nodes_per_keypoint, np.int64).reshape(-1)
    idx = np.flatnonzero(nodes >= 0)
    order = idx[np.argsort(nodes[idx], kind="stable")]
    node_id, counts = np.unique(nodes[idx], return_counts=True)
    node_start = np.concatenate([[0], np.cumsum(counts)]) if len(node_id) else np.zeros(1, np.int64)
    return node_id.astype(np.int32), node_start.astype(np.int32), order.astype(np.int32)


def epi_feats(kf):
    """The lba_epi_feat records of one keyframe from the mapping `tri_rows` takes (key_to_cam, keys_un, octave,
    global_to_local, u_right, level_sigma2, scale_factors) plus
      desc [N, 8] uint32 (or [N, 32] uint8, the rows of mvDescriptors)    angle   mvKeysUn[idx].angle
      has_point   GetMapPoint(idx) != NULL
    u_right is mvuRight[mmpGlobalToLocalID[idx]] where that exists, -1 otherwise (the stereo rule also asks for the last
    camera, which the kernel checks)."""
    cam = np.asarray(kf["key_to_cam"], np.int64)
    n = len(cam)
    f = np.zeros(n, EPI_FEAT_DTYPE)
    octave = np.asarray(kf["octave"], np.int64)
    local = np.asarray(kf["global_to_local"], np.int64)
    u_right = np.asarray(kf["u_right"], np.float32)
    has = (local >= 0) & (local < len(u_right))
    f["x"], f["y"] = np.asarray(kf["keys_un"], np.float32).reshape(n, 2).T
    f["angle"] = np.asarray(kf.get("angle", np.zeros(n)), np.float32)
    f["u_right"] = np.where(has, u_right[np.where(has, local, 0)] if len(u_right) else -1.0, np.float32(-1.0))
    f["scale"] = np.asarray(kf["scale_factors"], np.float32)[octave]
    f["sigma2"] = np.asarray(kf["level_sigma2"], np.float32)[octave]
    f["cam"] = cam
    f["has_point"] = np.asarray(kf.get("has_point", np.zeros(n)), bool)
    desc = np.ascontiguousarray(kf["desc"])
    f["desc"] = desc.view(np.uint32).reshape(n, 8) if desc.dtype == np.uint8 else np.asarray(desc, np.uint32).reshape(n, 8)
    return f


def pack_epi_keyframes(feats_per_kf, nodes_per_kf):
    """Several keyframes one behind the other: `feats_per_kf` their EPI_FEAT_DTYPE arrays, `nodes_per_kf` one node id
    per keypoint each.  Returns (ekfs, feats, node_id, node_start, node_feat); a keyframe has n_node + 1 rows of
    node_id / node_start (the last row of node_id is not read)."""
    ekfs = np.zeros(len(feats_per_kf), EPI_KF_DTYPE)
    ids, starts, nfs, f0, r0, n0 = [], [], [], 0, 0, 0
    for k, (f, nodes) in enumerate(zip(feats_per_kf, nodes_per_kf)):
        nid, ns, nf = feat_vec_csr(nodes)
        ekfs[k] = (f0, len(f), r0, len(nid), n0, 0)
        ids.append(np.concatenate([nid, [-1]]).astype(np.int32))
        starts.append(ns)
        nfs.append(nf)
        f0, r0, n0 = f0 + len(f), r0 + len(nid) + 1, n0 + len(nf)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
    feats = np.concatenate(feats_per_kf) if len(feats_per_kf) else np.zeros(0, EPI_FEAT_DTYPE)
    return ekfs, feats.astype(EPI_FEAT_DTYPE), cat(ids, np.int32), cat(starts, np.int32), cat(nfs, np.int32)


def epi_pairs(kf1, kf2, ekfs):
    """lba_epi_pair records for the keyframe indices kf1[i], kf2[i], their out ranges one behind the other"""
    kf1, kf2 = np.atleast_1d(np.asarray(kf1, np.int64)), np.atleast_1d(np.asarray(kf2, np.int64))
    pairs = np.zeros(len(kf1), EPI_PAIR_DTYPE)
    pairs["kf1"], pairs["kf2"] = kf1, kf2
    n1 = np.asarray(ekfs["n_feat"], np.int64)[kf1]
    pairs["out0"] = np.concatenate([[0], np.cumsum(n1)[:-1]]) if len(kf1) else 0
    return pairs


def epi_matches(pair, out, ekfs):
    """vMatchedPairs of one pair: [n, 2] (idx1, idx2) in ascending idx1, what tri_rows expects as `matches`"""
    rows = out[int(pair["out0"]):int(pair["out0"]) + int(ekfs[int(pair["kf1"])]["n_feat"])]
    idx1 = np.flatnonzero(rows["status"] == EPI_OK)
    return np.stack([idx1, rows["idx2"][idx1].astype(np.int64)], axis=1).reshape(-1, 2)


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def make_epi_pairs(n_pairs=1, n_cam=4, n_feat=400, n_nodes=40, seed=0, baselines=(1.0, 1.5, 2.0, 3.0), noise=0.5,
                   seen_frac=0.7, clutter_frac=0.6, bits=(0, 40), clutter_bits=(0, 30), has_point_frac=0.15,
                   no_node_frac=0.03, twin_frac=0.1, stereo_frac=0.7, stereo_b=0.12, depth_range=(3.0, 25.0), n_octaves=8):
    """Synthetic SearchForTriangulation inputs on the rig of make_tri_pairs (tri_rig / tri_keyframes: `n_cam` pinhole
    cameras, the LAST one looking ahead and stereo): a current keyframe (index 0) and `n_pairs` neighbours, each with
    `n_feat` keypoints per camera, camera-major.  Every keypoint of the current keyframe is a world point at a depth in
    `depth_range` with a random base descriptor; its own descriptor is the base with some of `bits` flipped
    (match.flip_bits), its vocabulary node comes from the BASE descriptor (base[0] % n_nodes), so partners mostly
    share a node; a share `no_node_frac` of keypoints is in no node.  A neighbour sees a share `seen_frac` of the points
    (in the camera that has it nearest its image centre, `noise` pixels of error, the octave following the distance
    ratio); its other keypoints are clutter: a share `clutter_frac` of them takes the base and the node of a random
    point with `clutter_bits` flipped but sits at a random place, off the epipolar line; a share `twin_frac` repeats a
    seen keypoint one octave up with the same descriptor (a tie); the rest is random.  A share
    `has_point_frac` of all keypoints has a map point; a share `stereo_frac` of the last camera's has u_right (and a
    depth).  Every value is rounded to float as the map holds it.
    Returns (pairs, kfs, ekfs, cams, feats, node_id, node_start, node_feat, truth) with truth = {"kf": the per-keyframe
    mappings for epi_feats / tri_rows, "nodes": node per keypoint, "partner": per neighbour the keypoint of it that
    shows point i or -1}."""
    rng = np.random.default_rng([seed, 0xE91])
    from .synth import _expso3, _rotz
    from .triangulate import _RBC0
    fx, fy, cx, cy = TRI_K
    W, H = 960.0, 600.0
    sf, sig2 = scale_pyramid(n_octaves)
    bf = float(np.float32(fx * stereo_b))
    N = n_cam * n_feat
    cur = (_rotz(rng.uniform(-np.pi, np.pi)) @ _RBC0, rng.uniform(-20, 20, 3))
    poses = [cur]
    for p in range(n_pairs):
        b = baselines[p % len(baselines)]
        d = cur[0] @ (np.array([np.cos(0.7 + 0.9 * p), 0.1, np.sin(0.7 + 0.9 * p)]) * b)
        poses.append((cur[0] @ _expso3(rng.normal(0, np.deg2rad(3.0), 3)), cur[1] + d))
    kfs, cams = tri_keyframes(poses, n_cam, stereo_b)
    pose = [[(C["Tcw"].reshape(3, 4)[:, :3], C["Tcw"].reshape(3, 4)[:, 3], C["Ow"]) for C in cams[k * n_cam:(k + 1) * n_cam]]
            for k in range(len(kfs))]

    def nbits(lo_hi):
        return int(rng.integers(lo_hi[0], lo_hi[1] + 1))

    def blank():
        return {"key_to_cam": np.zeros(N, np.int64), "keys_un": np.zeros((N, 2), np.float32), "octave": np.zeros(N, np.int64),
                "angle": np.zeros(N, np.float32), "desc": np.zeros((N, 8), np.uint32), "u_right_kp": np.full(N, -1.0, np.float32),
                "depth_kp": np.zeros(N, np.float32), "node": np.full(N, -1, np.int64),
                "has_point": rng.random(N) < has_point_frac}

    def stereo(kf, i, u, z):
        if kf["key_to_cam"][i] == n_cam - 1 and rng.random() < stereo_frac and z > 0.1:
            ur = np.float32(u - bf / z + rng.normal(0, noise * 0.5))
            disp = np.float32(u) - ur
            if ur >= 0 and disp > 0:
                kf["u_right_kp"][i], kf["depth_kp"][i] = ur, np.float32(bf) / disp

    k0 = blank()
    Xw, base, node = np.zeros((N, 3)), rng.integers(0, 2 ** 32, (N, 8), dtype=np.uint64).astype(np.uint32), np.zeros(N, np.int64)
    for i in range(N):
        c1 = i // n_feat
        R1, t1, _ = pose[0][c1]
        uv = np.array([rng.uniform(20, W - 20), rng.uniform(20, H - 20)])
        z = rng.uniform(*depth_range)
        Xw[i] = R1.T @ (np.array([(uv[0] - cx) / fx * z, (uv[1] - cy) / fy * z, z]) - t1)
        o = int(rng.integers(0, n_octaves))
        node[i] = int(base[i, 0]) % n_nodes
        k0["key_to_cam"][i], k0["octave"][i] = c1, o
        k0["keys_un"][i] = uv + rng.normal(0, noise, 2) * float(sf[o])
        k0["angle"][i] = rng.uniform(0, 360)
        k0["desc"][i] = flip_bits(base[i], nbits(bits), rng)
        k0["node"][i] = -1 if rng.random() < no_node_frac else node[i]
        stereo(k0, i, k0["keys_un"][i][0], z)
    maps, partners = [k0], []
    for p in range(n_pairs):
        kf, partner = blank(), np.full(N, -1, np.int64)
        rec, seen = [], []
        for i in range(N):
            best, c2, Y2 = np.inf, -1, None
            if rng.random() < seen_frac:
                for c in range(n_cam):
                    Y = pose[p + 1][c][0] @ Xw[i] + pose[p + 1][c][1]
                    if Y[2] > 0.1:
                        u, v = fx * Y[0] / Y[2] + cx, fy * Y[1] / Y[2] + cy
                        off = np.hypot(u - cx, v - cy)
                        if 0 <= u < W and 0 <= v < H and off < best:
                            best, c2, Y2 = off, c, Y
            if c2 >= 0:
                o1 = int(k0["octave"][i])
                ratio = np.linalg.norm(Xw[i] - pose[p + 1][c2][2]) / np.linalg.norm(Xw[i] - pose[0][i // n_feat][2])
                o = int(np.clip(o1 - np.round(np.log(ratio) / np.log(1.2)), 0, n_octaves - 1))
                uv = np.array([fx * Y2[0] / Y2[2] + cx, fy * Y2[1] / Y2[2] + cy]) + rng.normal(0, noise, 2) * float(sf[o])
                seen.append(len(rec))
                rec.append((c2, i, uv, o, (k0["angle"][i] + rng.normal(0, 5.0)) % 360.0, flip_bits(base[i], nbits(bits), rng),
                            node[i], Y2[2]))
            elif seen and rng.random() < twin_frac:      # the same corner found once more, one octave up: a tie
                c, src, uv, o, ang, d, nd, z = rec[seen[int(rng.integers(0, len(seen)))]]
                rec.append((c, -1, uv + rng.normal(0, 0.3, 2), min(o + 1, n_octaves - 1), ang, d.copy(), nd, z))
            else:
                j = int(rng.integers(0, N))
                near = rng.random() < clutter_frac
                d = flip_bits(base[j], nbits(clutter_bits), rng) if near else rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
                uv = np.array([rng.uniform(0, W), rng.uniform(0, H)])
                rec.append((int(rng.integers(0, n_cam)), -1, uv, int(rng.integers(0, n_octaves)), rng.uniform(0, 360), d,
                            node[j] if near else int(d[0]) % n_nodes, rng.uniform(*depth_range)))
        rec.sort(key=lambda r: r[0])       # camera-major, stable
        for i, (c, src, uv, o, ang, d, nd, z) in enumerate(rec):
            kf["key_to_cam"][i], kf["octave"][i], kf["keys_un"][i], kf["angle"][i], kf["desc"][i] = c, o, uv, ang, d
            kf["node"][i] = -1 if rng.random() < no_node_frac else nd
            if src >= 0:
                partner[src] = i
            stereo(kf, i, kf["keys_un"][i][0], z)
        maps.append(kf)
        partners.append(partner)
    for kf in maps:     # the remaining fields of the mapping tri_rows / epi_feats take
        cam = kf["key_to_cam"]
        kf["keys"] = kf["keys_un"]
        kf["global_to_local"] = np.arange(N) - np.searchsorted(cam, cam)      # the index within its camera
        last = cam == n_cam - 1
        kf["u_right"], kf["depth"] = kf["u_right_kp"][last], kf["depth_kp"][last]
        kf["level_sigma2"], kf["scale_factors"] = sig2, sf
    ekfs, feats, node_id, node_start, node_feat = pack_epi_keyframes([epi_feats(kf) for kf in maps], [kf["node"] for kf in maps])
    pairs = epi_pairs(np.zeros(n_pairs, np.int64), 1 + np.arange(n_pairs), ekfs)
    truth = {"kf": maps, "nodes": [kf["node"] for kf in maps], "partner": partners, "X": Xw}
    return pairs, kfs, ekfs, cams, feats, node_id, node_start, node_feat, truth
