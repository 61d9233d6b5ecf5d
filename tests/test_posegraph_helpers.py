"""amc_lba.posegraph.essential_graph and write_back (the caller's side of Optimizer::OptimizeEssentialGraph,
src/Optimizer.cc:1465-1660 and :1669-1713) on a hand-made map of eight keyframes, rule by rule, and on the synthetic
map of make_pose_graph.  CPU only."""
import numpy as np

from amc_lba.posegraph import MIN_FEAT, essential_graph, make_pose_graph, s_inv, s_map, s_mul, s_of, write_back
from amc_lba.synth import _rotz


# A float-valued rotation matrix is orthonormal to 1e-7 only and a record carries the unit quaternion made from it (as
# Tcw.unit_quaternion() does in the reference): compared poses agree to that, times a lever of up to 20 m.  What the
# tests tell apart is the loop's correction: 0.03 rad and 0.4 m.
TOL = 1e-5


def _pose(k):
    """Tiw of keyframe k: 2 m apart along x, a slow yaw; float values as GetPose() gives them."""
    R = _rotz(0.1 * k).astype(np.float32).astype(np.float64)
    return R, np.array([-2.0 * k, 0.5 * k, 0.0], np.float32).astype(np.float64)


def _map():
    ids = np.array([0, 1, 2, 3, 5, 6, 8, 9])                      # mnIds with gaps; 5 is bad
    n = len(ids)
    row = {int(k): i for i, k in enumerate(ids)}
    bad = np.zeros(n, bool)
    bad[row[5]] = True
    parent = np.array([-1, 0, 1, 2, 3, 3, 6, 8])                  # 6's parent is 3 (5 is bad); 8 <- 6, 9 <- 8
    covis = [[] for _ in range(n)]

    def link(a, b, w):
        covis[row[a]].append((b, w))
        covis[row[b]].append((a, w))
    link(0, 1, 300); link(1, 2, 300); link(2, 3, 300); link(3, 6, 250); link(6, 8, 300); link(8, 9, 300)
    link(0, 2, 150)        # a plain covisibility edge: 2 -> 0
    link(1, 3, 99)         # below minFeat: no edge
    link(3, 5, 200)        # to a bad keyframe: no edge
    link(2, 6, 120)        # 6 -> 2
    link(9, 0, 180)        # the loop pair itself: in sInsertedEdges, so not again as a covisibility edge
    link(9, 1, 130)        # a loop connection above minFeat
    link(8, 0, 40)         # a loop connection below minFeat: dropped
    link(8, 1, 110)        # covisible, but also a loop connection: inserted once, by the loop connections
    covis = [sorted(c, key=lambda kw: -kw[1]) for c in covis]
    pose = [_pose(int(k)) for k in ids]
    S = lambda k: (pose[row[k]][0], pose[row[k]][1], 1.0)         # noqa: E731
    corr = (_rotz(0.03), np.array([0.4, -0.2, 0.0]), 1.0)         # the loop's correction, applied on the right
    corrected = {k: s_mul(S(k), corr) for k in (8, 9)}
    non_corrected = {k: S(k) for k in (8, 9)}
    return dict(ids=ids, bad=bad, pose=pose, init_id=0, parent=parent, loop_edges={6: {1}, 1: {6}}, covis=covis,
                corrected=corrected, non_corrected=non_corrected,
                loop_connections={9: {0, 1}, 8: {0, 1}}, cur_id=9, loop_id=0), S


def _edges(e, vids):
    return [(int(vids[a]), int(vids[b])) for a, b in zip(e["v0"], e["v1"])]


def test_vertices():
    m, S = _map()
    v, e, vids = essential_graph(m)
    assert vids.tolist() == [0, 1, 2, 3, 6, 8, 9]                                  # the bad one has no vertex
    assert v["fixed"].tolist() == [1, 0, 0, 0, 0, 0, 0]                            # the map's initial keyframe
    for k in (0, 3, 6):                                                            # GetPose(), scale 1
        R, t, s = s_of(v[vids.tolist().index(k)])
        assert np.abs(R - S(k)[0]).max() < TOL and np.abs(t - S(k)[1]).max() < TOL and s == 1.0
    for k in (8, 9):                                                               # CorrectedSim3
        R, t, _ = s_of(v[vids.tolist().index(k)])
        assert np.abs(R - m["corrected"][k][0]).max() < TOL and np.abs(t - m["corrected"][k][1]).max() < TOL


def test_edge_rules_and_order():
    m, _ = _map()
    v, e, vids = essential_graph(m)
    got = _edges(e, vids)
    want = [
        (8, 1),                    # loop connections in key order: 8 -> {0: weight 40 < minFeat, dropped; 1}
        (9, 0), (9, 1),            # 9 -> {0: the pair (current, loop) passes whatever its weight; 1}
        (1, 0),                    # then per keyframe: spanning tree,
        (2, 1), (2, 0),            #   covisibles of weight >= minFeat with a lower id (1 is its parent)
        (3, 2),                    #   (3 - 1: 99 < minFeat)
        (6, 3), (6, 1), (6, 2),    #   spanning tree, the earlier loop edge 6 -> 1 (1 -> 6 has the higher id), covisible 2
        (8, 6),                    #   (8 - 1 is in sInsertedEdges; 8 - 0 is below minFeat)
        (9, 8),                    #   (9 - 0 and 9 - 1 are in sInsertedEdges)
    ]
    assert got == want
    assert MIN_FEAT == 100
    assert all(5 not in p for p in got)                                            # nothing to the bad keyframe


def test_measurements():
    m, S = _map()
    v, e, vids = essential_graph(m)
    got = _edges(e, vids)
    vS = {int(k): s_of(v[i]) for i, k in enumerate(vids)}

    def meas(i, j):
        return s_of(e[got.index((i, j))])

    def same(A, B):
        return np.abs(A[0] - B[0]).max() < TOL and np.abs(A[1] - B[1]).max() < TOL and abs(A[2] - B[2]) < TOL
    assert same(meas(9, 0), s_mul(vS[0], s_inv(vS[9])))          # a loop connection: the vertices' estimates (corrected)
    assert same(meas(9, 8), s_mul(S(8), s_inv(S(9))))            # both ends non-corrected: the odometry as it was
    assert same(meas(8, 6), s_mul(S(6), s_inv(S(8))))            # one end non-corrected, the other its pose
    assert same(meas(2, 0), s_mul(S(0), s_inv(S(2))))
    # so at the start the error of a normal edge between an uncorrected and a corrected keyframe is the correction
    assert not same(meas(8, 6), s_mul(vS[6], s_inv(vS[8])))


def test_write_back():
    m, _ = _map()
    v, e, vids = essential_graph(m)
    opt = v.copy()
    opt["t"][3] += [0.25, -0.5, 0.125]
    opt["s"][5] = 1.25                                            # keyframe 8 comes back with a scale
    m.update(points=np.array([[1.5, 2.0, 8.0], [-3.0, 0.5, 6.0], [0.0, 0.0, 5.0], [2.0, 1.0, 4.0]], np.float32),
             point_bad=np.array([False, False, True, False]), point_ref=np.array([3, 8, 3, 2]),
             point_corrected_by=np.array([-1, 9, -1, 4]), point_corrected_ref=np.array([0, 9, 0, 0]))
    poses, pts = write_back(m, v, opt, vids)
    assert sorted(poses) == vids.tolist()
    R8, t8, s8 = s_of(opt[5])
    assert poses[8][0].dtype == np.float32 and poses[8][1].dtype == np.float32
    np.testing.assert_array_equal(poses[8][0], R8.astype(np.float32))
    np.testing.assert_array_equal(poses[8][1], t8.astype(np.float32) / np.float32(1.25))      # [R, t / s] in float
    # point 0: through its reference keyframe 3, which moved; point 1: corrected by the current keyframe, so through
    # mnCorrectedReference = 9, which did not move (back to itself up to float); point 2 is bad: untouched bitwise;
    # point 3: corrected by another keyframe (4 != current), so through its own reference 2
    X0 = s_map(s_inv(s_of(opt[3])), s_map(s_of(v[3]), m["points"][0].astype(np.float64)))
    np.testing.assert_array_equal(pts[0], X0.astype(np.float32))
    assert np.abs(pts[0] - m["points"][0]).max() > 0.1
    assert np.abs(pts[1] - m["points"][1]).max() < 1e-5
    assert pts[2].tobytes() == m["points"][2].tobytes()
    assert np.abs(pts[3] - m["points"][3]).max() < 1e-5
    assert pts.dtype == np.float32


def test_synthetic_map():
    m = make_pose_graph(n_kf=40, seed=2, n_points=50, old_loop=True)
    v, e, vids = essential_graph(m)
    assert len(v) == 40 and v["fixed"].sum() == 1 and v["fixed"][0] == 1
    pairs = _edges(e, vids)
    assert pairs[0][0] in (m["cur_id"], m["cur_id"] - 2)                           # the loop connections come first
    assert (m["cur_id"], m["loop_id"]) in pairs
    assert (int(vids[13]), int(vids[2])) in pairs                                  # the earlier loop edge, once
    assert (int(vids[2]), int(vids[13])) not in pairs
    assert sum(1 for a, b in pairs if (a, b) == (m["cur_id"] - 2, m["loop_id"])) == 0   # weight 60 < minFeat
    assert len(pairs) > 39 + 30                                                    # a spanning tree and covisibility
    poses, pts = write_back(m, v, v, vids)                                         # nothing optimised: points stay
    keep = ~m["point_bad"]
    assert np.abs(pts[keep] - m["points"][keep]).max() < 1e-4
