"""MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:611-700) and MapPoint::ComputeDistinctiveDescriptors (:498-578)
restated twice in numpy, for the tests of lba_mappoint_refresh.

`refresh_loops` is the loops as written, with float32 scalars and Python integers: the candidates in list order, the
matrix, a sort per row, the element at int(0.5 * (N - 1)), the first strict minimum; the sum of unit vectors one
observation after the other.  `refresh_vec` is vectorised: the distance matrix by two matrix products of the bit
planes, np.sort, the first argmin; the unit vectors at once and np.add.accumulate (strictly sequential) for the sum;
fmax / fmin for the range.  Both take a point record and return a copy with what the call would leave in it.

`MISTAKES` are six ways to get it wrong (keyword switches of refresh_loops); tests/test_mp_cases.py counts the rows of
the generated problems each would change.
"""
import numpy as np

from amc_lba.abi import MP_POINT_DTYPE
from amc_lba.mappoint import MP_BAD, MP_DESC, MP_EMPTY, MP_NORMAL, MP_OK

F = np.float32
FLT_MIN, FLT_MAX = np.finfo(F).tiny, np.finfo(F).max
MISTAKES = ("upper_median", "ties_last", "skip_bad_in_normal", "tree_sum", "mul_inv", "fma_norm")
OUT_FIELDS = ("normal", "min_distance", "max_distance", "desc", "n", "best_obs", "best_median", "status")


def _begin(P):
    R = np.array(P, MP_POINT_DTYPE).copy().reshape(())
    R["n"], R["best_obs"], R["best_median"] = 0, -1, -1
    R["status"] = MP_BAD if P["bad"] else MP_EMPTY if P["n_obs"] == 0 else MP_OK
    return R


def _list(P, obs):
    return obs[int(P["obs0"]):int(P["obs0"]) + int(P["n_obs"])]


def _is_bad(kf_bad, kf):
    return kf_bad is not None and bool(kf_bad[kf])


def _tree(v):
    if len(v) == 1:
        return v[0]
    h = len(v) // 2
    return _tree(v[:h]) + _tree(v[h:])


def refresh_loops(P, obs, K, kf_bad=None, scale_top=None, upper_median=False, ties_last=False,
                  skip_bad_in_normal=False, tree_sum=False, mul_inv=False, fma_norm=False):
    R = _begin(P)
    if R["status"] != MP_OK:
        return R
    top = F(K.scale_top if scale_top is None else scale_top)
    L = _list(P, obs)
    if int(P["ops"]) & MP_DESC:
        cand = [k for k in range(len(L)) if not _is_bad(kf_bad, L[k]["kf"])]
        if cand:
            ints = [int.from_bytes(K.feature(L[k]["kf"], L[k]["feat"])["desc"].tobytes(), "little") for k in cand]
            N = len(ints)
            D = [[0] * N for _ in range(N)]
            for i in range(N):
                for j in range(i + 1, N):
                    D[i][j] = D[j][i] = (ints[i] ^ ints[j]).bit_count()
            m = int(0.5 * N) if upper_median else int(0.5 * (N - 1))
            best, best_i = 2 ** 31 - 1, 0
            for i in range(N):
                med = sorted(D[i])[m]
                if med < best or (ties_last and med == best):
                    best, best_i = med, i
            k = cand[best_i]
            R["desc"] = K.feature(L[k]["kf"], L[k]["feat"])["desc"]
            R["best_obs"], R["best_median"] = k, best
    if int(P["ops"]) & MP_NORMAL:
        pos = [F(x) for x in P["pos"]]
        units, n = [], 0
        maxd, mind = F(FLT_MIN), F(FLT_MAX)
        with np.errstate(all="ignore"):
            for o in L:
                ft = K.feature(o["kf"], o["feat"])
                ow = K.centre(o["kf"], ft["cam"])
                d = [pos[i] - ow[i] for i in range(3)]
                if fma_norm:       # fma(dz, dz, fma(dy, dy, dx * dx)): the products unrounded (exact in float64)
                    t = F(np.float64(d[1]) * np.float64(d[1]) + np.float64(d[0] * d[0]))
                    r = np.sqrt(F(np.float64(d[2]) * np.float64(d[2]) + np.float64(t)))
                else:
                    r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                if o["kf"] == P["ref_kf"]:
                    a, b = r * ft["scale"], r * ft["scale"] / top
                    if maxd < a:
                        maxd = a
                    if b < mind:
                        mind = b
                if skip_bad_in_normal and _is_bad(kf_bad, o["kf"]):
                    continue
                inv = F(1) / r
                units.append([d[i] * inv if mul_inv else d[i] / r for i in range(3)])
                n += 1
            normal = [F(0), F(0), F(0)]
            if tree_sum and units:
                normal = [F(0) + _tree([u[i] for u in units]) for i in range(3)]
            else:
                for u in units:
                    normal = [normal[i] + u[i] for i in range(3)]
            R["normal"] = [normal[i] / F(n) for i in range(3)]
        R["max_distance"], R["min_distance"], R["n"] = maxd, mind, n
    return R


def distance_matrix(descs):
    """[N, N] Hamming distances of [N, 8] uint32 descriptors: a (1 - b)^T + (1 - a) b^T on the bit planes (exact)"""
    bits = np.unpackbits(np.ascontiguousarray(descs, np.uint32).view(np.uint8), axis=1).astype(F)
    return (bits @ (1 - bits).T + (1 - bits) @ bits.T).astype(np.int64)


def refresh_vec(P, obs, K, kf_bad=None, scale_top=None):
    R = _begin(P)
    if R["status"] != MP_OK:
        return R
    top = F(K.scale_top if scale_top is None else scale_top)
    L = _list(P, obs)
    ft = K.feats[K.ekfs["feat0"][L["kf"]] + L["feat"]]
    if int(P["ops"]) & MP_DESC:
        cand = np.arange(len(L)) if kf_bad is None else np.flatnonzero(np.asarray(kf_bad)[L["kf"]] == 0)
        if len(cand):
            D = np.sort(distance_matrix(ft["desc"][cand]), axis=1)
            med = D[:, int(0.5 * (len(cand) - 1))]
            i = int(np.argmin(med))      # the first of the least
            R["desc"] = ft["desc"][cand[i]]
            R["best_obs"], R["best_median"] = cand[i], med[i]
    if int(P["ops"]) & MP_NORMAL:
        ow = K.cams["Ow"][K.kfs["cam0"][L["kf"]] + ft["cam"]].astype(F)
        with np.errstate(all="ignore"):
            d = P["pos"].astype(F)[None, :] - ow
            r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=F)
            acc = np.add.accumulate(np.vstack([np.zeros((1, 3), F), d / r[:, None]]), axis=0, dtype=F)[-1]
            R["normal"] = acc / F(len(L))
            ref = L["kf"] == P["ref_kf"]
            a = r[ref] * ft["scale"][ref]
            b = r[ref] * ft["scale"][ref] / top
            R["max_distance"] = np.fmax.reduce(np.concatenate([[F(FLT_MIN)], a]).astype(F))
            R["min_distance"] = np.fmin.reduce(np.concatenate([[F(FLT_MAX)], b]).astype(F))
        R["n"] = len(L)
    return R


def refresh_batch(points, obs, K, kf_bad=None, scale_top=None, form=refresh_vec, **kw):
    out = np.array(points, MP_POINT_DTYPE).copy()
    for i in range(len(out)):
        out[i] = form(points[i], obs, K, kf_bad, scale_top, **kw)[()]
    return out


def same_float(a, b):
    """float32 arrays identical in their bits, a NaN matching any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def diff_fields(got, want):
    """the out fields in which two records (or arrays of records) differ; every other field must be byte-identical"""
    out = []
    for f in MP_POINT_DTYPE.names:
        if f == "pad":
            continue
        if f in ("normal", "min_distance", "max_distance"):
            ok = same_float(got[f], want[f])
        else:
            ok = np.asarray(got[f]).tobytes() == np.asarray(want[f]).tobytes()
        if not ok:
            out.append(f)
    return out
