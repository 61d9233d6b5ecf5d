"""numpy dtypes that mirror the C structs of include/amc_lba.h byte for byte.

Used both by the ctypes binding of the product (`amc_lba.Problem`) and by the oracle
binding under oracle/ (test infrastructure), so both sides read identical buffers.
"""
import ctypes

import numpy as np

KF_DTYPE = np.dtype([
    ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("vel", "<f8", (6,)),
    ("time", "<f8"), ("bf", "<f8"), ("fixed", "<i4"), ("pad", "<i4"),
], align=True)

OBS_DTYPE = np.dtype([
    ("kind", "<i4"), ("kf_a", "<i4"), ("kf_b", "<i4"), ("lm", "<i4"), ("cam", "<i4"), ("pad", "<i4"),
    ("t", "<f8"), ("z", "<f8", (3,)), ("w", "<f8"),
], align=True)

PRIOR_DTYPE = np.dtype([("kf_a", "<i4"), ("kf_b", "<i4")], align=True)

CAM_DTYPE = np.dtype([
    ("q", "<f8", (4,)), ("t", "<f8", (3,)),
    ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"),
    ("ext_free", "<i4"), ("pad", "<i4"), ("rbc_ini", "<f8", (4,)), ("rbc_info", "<f8", (9,)),
], align=True)

# lba_triangulate (CreateNewMapPoints)
TRI_CAM_DTYPE = np.dtype([
    ("Tcw", "<f8", (12,)), ("Ow", "<f8", (3,)),
    ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"), ("invfx", "<f8"), ("invfy", "<f8"),
], align=True)
TRI_KF_DTYPE = np.dtype([
    ("Rwb", "<f8", (9,)), ("twb", "<f8", (3,)), ("bf", "<f8"), ("b", "<f8"), ("cam0", "<i4"), ("pad", "<i4"),
], align=True)
TRI_ROW_DTYPE = np.dtype([
    ("cam1", "<i4"), ("cam2", "<i4"), ("status", "<i4"), ("stereo_point", "<i4"),
    ("z1", "<f8", (2,)), ("z2", "<f8", (2,)), ("k1", "<f8", (2,)), ("k2", "<f8", (2,)),
    ("ur1", "<f8"), ("ur2", "<f8"), ("depth1", "<f8"), ("depth2", "<f8"),
    ("sigma2_1", "<f8"), ("sigma2_2", "<f8"), ("scale1", "<f8"), ("scale2", "<f8"), ("X", "<f8", (3,)),
], align=True)
TRI_PAIR_DTYPE = np.dtype([
    ("kf1", "<i4"), ("kf2", "<i4"), ("row0", "<i4"), ("n_rows", "<i4"), ("n_new", "<i4"), ("n_stereo", "<i4"),
], align=True)
assert TRI_CAM_DTYPE.itemsize == 168
assert TRI_KF_DTYPE.itemsize == 120
assert TRI_ROW_DTYPE.itemsize == 168
assert TRI_PAIR_DTYPE.itemsize == 24

# lba_match_epipolar (ORBmatcher::SearchForTriangulation); it shares TRI_KF_DTYPE / TRI_CAM_DTYPE
EPI_FEAT_DTYPE = np.dtype([
    ("x", "<f4"), ("y", "<f4"), ("angle", "<f4"), ("u_right", "<f4"), ("scale", "<f4"), ("sigma2", "<f4"),
    ("cam", "<i4"), ("has_point", "<i4"), ("desc", "<u4", (8,)),
], align=True)
EPI_KF_DTYPE = np.dtype([
    ("feat0", "<i4"), ("n_feat", "<i4"), ("node0", "<i4"), ("n_node", "<i4"), ("nf0", "<i4"), ("pad", "<i4"),
], align=True)
EPI_PAIR_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("out0", "<i4"), ("n_matches", "<i4")], align=True)
EPI_ROW_DTYPE = np.dtype([("idx2", "<i4"), ("dist", "<i4"), ("status", "<i4"), ("pad", "<i4")], align=True)
assert EPI_FEAT_DTYPE.itemsize == 64
assert EPI_KF_DTYPE.itemsize == 24
assert EPI_PAIR_DTYPE.itemsize == 16
assert EPI_ROW_DTYPE.itemsize == 16

# lba_match_bow (ORBmatcher::SearchByBoW): the keyframe arrays are lba_match_epipolar's
BOW_PAIR_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("out0", "<i4"), ("n_matches", "<i4")], align=True)
BOW_ROW_DTYPE = np.dtype([("idx2", "<i4"), ("dist", "<i4"), ("dist2", "<i4"), ("status", "<i4")], align=True)
assert BOW_PAIR_DTYPE.itemsize == 16
assert BOW_ROW_DTYPE.itemsize == 16

# lba_match_project (ORBmatcher::SearchByProjection)
MATCH_CAM_DTYPE = np.dtype([
    ("min_x", "<f4"), ("min_y", "<f4"), ("grid_w_inv", "<f4"), ("grid_h_inv", "<f4"), ("rounds", "<i4"),
], align=True)
MATCH_FEAT_DTYPE = np.dtype([
    ("x", "<f4"), ("y", "<f4"), ("angle", "<f4"), ("u_right", "<f4"), ("octave", "<i4"), ("cam", "<i4"),
    ("taken", "<i4"), ("job", "<i4"), ("desc", "<u4", (8,)),
], align=True)
MATCH_JOB_DTYPE = np.dtype([
    ("x", "<f4"), ("y", "<f4"), ("radius", "<f4"), ("ur", "<f4"), ("angle", "<f4"), ("cam", "<i4"),
    ("min_level", "<i4"), ("max_level", "<i4"), ("point", "<i4"), ("blocks", "<i4"), ("desc", "<u4", (8,)),
    ("feat", "<i4"), ("status", "<i4"), ("best_dist", "<i4"), ("best_dist2", "<i4"), ("pad", "<i4", (2,)),
], align=True)
MATCH_SEARCH_DTYPE = np.dtype([
    ("cam0", "<i4"), ("n_cam", "<i4"), ("feat0", "<i4"), ("n_feat", "<i4"), ("job0", "<i4"), ("n_jobs", "<i4"),
    ("cell0", "<i4"), ("cf0", "<i4"), ("n_matches", "<i4"), ("n_matches_mono", "<i4"),
], align=True)
assert MATCH_CAM_DTYPE.itemsize == 20
assert MATCH_FEAT_DTYPE.itemsize == 64
assert MATCH_JOB_DTYPE.itemsize == 96
assert MATCH_SEARCH_DTYPE.itemsize == 40

# lba_match_fuse (ORBmatcher::Fuse's search); the points are lba_match_sim3_project's (sim3_project.S3P_POINT_DTYPE)
FUSE_CAM_DTYPE = np.dtype([
    ("q_cw", "<f4", (4,)), ("t_cw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
    ("min_x", "<f4"), ("max_x", "<f4"), ("min_y", "<f4"), ("max_y", "<f4"), ("ow", "<f4", (3,)),
], align=True)
FUSE_TARGET_DTYPE = np.dtype([
    ("cam0", "<i4"), ("n_cam", "<i4"), ("feat0", "<i4"), ("n_feat", "<i4"), ("cell0", "<i4"), ("cf0", "<i4"),
    ("bf", "<f4"), ("log_scale_factor", "<f4"), ("n_levels", "<i4"), ("sf0", "<i4"), ("sigma0", "<i4"), ("pad", "<i4"),
], align=True)
FUSE_SEARCH_DTYPE = np.dtype([
    ("target", "<i4"), ("point0", "<i4"), ("n_points", "<i4"), ("row0", "<i4"), ("mode", "<i4"), ("th", "<f4"),
    ("n_ok", "<i4"), ("pad", "<i4"),
], align=True)
FUSE_ROW_DTYPE = np.dtype([
    ("status", "<i4"), ("feat", "<i4"), ("best_dist", "<i4"), ("level", "<i4"), ("x", "<f4"), ("y", "<f4"),
    ("radius", "<f4"), ("n_cand", "<i4"),
], align=True)
assert FUSE_CAM_DTYPE.itemsize == 72
assert FUSE_TARGET_DTYPE.itemsize == 48
assert FUSE_SEARCH_DTYPE.itemsize == 32
assert FUSE_ROW_DTYPE.itemsize == 32

# lba_mappoint_refresh (MapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors); the keyframe arrays are
# lba_match_epipolar's
MP_OBS_DTYPE = np.dtype([("kf", "<i4"), ("feat", "<i4")], align=True)
MP_POINT_DTYPE = np.dtype([
    ("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"),
    ("desc", "<u4", (8,)), ("ref_kf", "<i4"), ("obs0", "<i4"), ("n_obs", "<i4"), ("bad", "<i4"), ("ops", "<i4"),
    ("n", "<i4"), ("best_obs", "<i4"), ("best_median", "<i4"), ("status", "<i4"), ("pad", "<i4", (3,)),
], align=True)
assert MP_OBS_DTYPE.itemsize == 8
assert MP_POINT_DTYPE.itemsize == 112

assert KF_DTYPE.itemsize == 128
assert OBS_DTYPE.itemsize == 64
assert PRIOR_DTYPE.itemsize == 8
assert CAM_DTYPE.itemsize == 200

# observation kinds (LBA_MONO_GP ... LBA_STEREO)
MONO_GP, STEREO_GP, MONO, STEREO = 0, 1, 2, 3

# status codes
LBA_OK, LBA_E_EMPTY, LBA_E_SOLVE, LBA_E_DIVERGED, LBA_E_ARG, LBA_E_HIP, LBA_E_LIMIT = 0, -1, -2, -3, -4, -5, -6
LBA_E_TIMEOUT = -7


class LbaConfig(ctypes.Structure):
    _fields_ = [
        ("qc", ctypes.c_double * 36),
        ("huber_mono", ctypes.c_double),
        ("huber_stereo", ctypes.c_double),
        ("huber_prior", ctypes.c_double),
        ("lambda_init", ctypes.c_double),
        ("tau", ctypes.c_double),
        ("max_trials", ctypes.c_int32),
        ("early_stop", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("flags", ctypes.c_int32),
    ]


class LbaStats(ctypes.Structure):
    _fields_ = [
        ("iterations", ctypes.c_int32),
        ("trials", ctypes.c_int32),
        ("result", ctypes.c_int32),
        ("solve_failures", ctypes.c_int32),
        ("chi2_initial", ctypes.c_double),
        ("chi2_final", ctypes.c_double),
        ("lambda_final", ctypes.c_double),
        ("ms_linearize", ctypes.c_double),
        ("ms_schur", ctypes.c_double),
        ("ms_solve", ctypes.c_double),
        ("ms_update_eval", ctypes.c_double),
        ("ms_total", ctypes.c_double),
        ("ms_k_linearize", ctypes.c_double),
        ("n_k_linearize", ctypes.c_int32),
        ("n_k_solve", ctypes.c_int32),
        ("ms_k_solve", ctypes.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# lba_config.flags (include/amc_lba.h)
FLAG_TIME_SWEEP = 1
FLAG_TIME_PHASES = 2
FLAG_HOST_LOOP = 4         # host-driven LM loop (default: queued trials decided on the device)
FLAG_BAND_SOLVE = 8        # reduced system solved by substitution after the factorisation (large systems)
FLAG_DENSE_SOLVE = 16      # force the L^-1-tile solve
FLAG_TIME_SAMPLED = 32     # with FLAG_TIME_SWEEP (queued loop): events on every 10th trial only
FLAG_SUBTREE_SOLVE = 64    # partitioned: distributed factorisation (window split by lba_partition_assign)
FLAG_F32_RESIDUAL = 128    # per-observation projection / residual / Jacobian rows in fp32, sums in fp64


def make_config(qc_diag=(0.02, 0.02, 0.02, 0.002, 0.002, 0.002), huber_mono=None, huber_stereo=None,
                huber_prior=0.0, lambda_init=1.0, tau=1e-5, max_trials=10, early_stop=1, device=0, flags=0):
    """LocalGPBA defaults: Huber deltas are float sqrt(5.991)/sqrt(7.815) widened to double
    (src/Optimizer.cc:975-978), lambda0 = 1.0 (:848-856), tau 1e-5, 10 trials."""
    cfg = LbaConfig()
    qc = np.zeros((6, 6))
    if np.ndim(qc_diag) == 2:
        qc[:] = qc_diag
    else:
        qc[np.diag_indices(6)] = qc_diag
    for i, v in enumerate(qc.ravel()):
        cfg.qc[i] = float(v)
    cfg.huber_mono = float(np.float32(np.sqrt(5.991))) if huber_mono is None else huber_mono
    cfg.huber_stereo = float(np.float32(np.sqrt(7.815))) if huber_stereo is None else huber_stereo
    cfg.huber_prior = huber_prior
    cfg.lambda_init = lambda_init
    cfg.tau = tau
    cfg.max_trials = max_trials
    cfg.early_stop = early_stop
    cfg.device = device
    cfg.flags = flags
    return cfg


def ptr(a, ctype=ctypes.c_void_p):
    """ctypes pointer to a C-contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctype)
